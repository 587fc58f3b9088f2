// Space-time p-norm stress aggregate of the transient path and its partial derivatives, gfx950, fp64.
//
//   S(t, W) = sum_{i < T} P_i,   P_i = 1/alpha [ int (m vm_top(w_i; t))^rho dx_4 + regc int t^rho dx_4 ]
//
// i.e. the sum over the time levels of PlateSim.pnorm_stress(level=i) (femo_alpha/dynamic_rm_shell/plate_sim.py:427-449) on the
// degree-4 measure of k_pnorm (tab_s).  The constraint of ex_gust_response_opt.py:320,329 and ex_lpc_gust_response_opt.py:49,55,445.
//
// k_stress_history: one thread per (cell, group of levels); the cell's element data (vertex coordinates, node indices, nodal h/E/nu)
// is loaded once and reused for every level of its group, grid.y runs over the level groups.  The quadrature-point geometry is
// re-derived per level from the registers rather than held for all points (nine QPG records would spill).
// GRAD = false: values only.  Results, none through float atomics:
//   bsum[l * gridDim.x + blockIdx.x]            the block's share of the level-l integral (fixed-order wave / block sum)
//   grad: ybuf[((l - l0) nel + pos) YSTRIDE]     scale * d P / d w_e of level l, cell slot pos of the Morton order (k_hist_gather)
//         tbuf[(blockIdx.y nel + e) NVC + b]     scale * d/dh of the group's levels, vertex b (entry 0 for per-cell thickness)
// Zero stress contributes zero (the convention of k_pnorm), so level 0 adds only the regularisation term.
#pragma once
#include "shell_device.h"
#include "stress.h"

namespace femo {

// block sum stored to *dst (no atomics): waves in a fixed order; every thread of the block must call it
__device__ __forceinline__ void block_sum_store(double v, double* dst) {
    __shared__ double s_part[16];
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) s_part[wid] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        const int nw = (blockDim.x + 63) >> 6;
        for (int i = 0; i < nw; ++i) t += s_part[i];
        *dst = t;
    }
    __syncthreads();
}

template <int NPC, int NVC, bool QUAD, bool UHAT, bool GRAD>
__global__ void __launch_bounds__(128)
k_stress_history(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const int* __restrict__ eorder, const double* __restrict__ H,
                 int64_t ldh, int l0, int nlev, int lpg, double ms, double rho, double scale, double regc,
                 double* __restrict__ bsum, double* __restrict__ ybuf, double* __restrict__ tbuf) {
    constexpr int LD = 3 * NPC + 3 * NVC;
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = pos < m.nel ? eorder[pos] : 0;
    const bool act = pos < m.nel && cell_selected(m, e);
    const int lb = l0 + blockIdx.y * lpg, le = min(l0 + nlev, lb + lpg);
    Elem<NPC, NVC> el;
    if (act) load_elem<NPC, NVC, UHAT>(m, f, e, el);
    double ge[NVC];
    for (int b = 0; b < NVC; ++b) ge[b] = 0.0;
    const bool ewm = f.ewm != 0;
    for (int l = lb; l < le; ++l) {             // uniform over the block: every thread reaches block_sum_store
        double acc = 0.0;
        double ye[LD];
        if (act) {
            const double* w = H + (size_t)l * ldh;
            double xe[LD];
            for (int a = 0; a < NPC; ++a)
                for (int c = 0; c < 3; ++c) xe[3 * a + c] = w[3 * el.pid[a] + c];
            for (int b = 0; b < NVC; ++b)
                for (int c = 0; c < 3; ++c) xe[3 * NPC + 3 * b + c] = w[m.ndof_u + 3 * rot_node(m, el, b) + c];
            if (GRAD)
                for (int i = 0; i < LD; ++i) ye[i] = 0.0;
            const int nq = tab->nq;
            for (int q = 0; q < nq; ++q) {
                QPG g;
                qp_geometry<NVC, QUAD, UHAT>(el.X, el.Uh, tab->N1[q], tab->dN1[q], g);
                const double wj = tab->w[q] * g.det * g.Ju;
                const double hq = interp<NVC>(tab->N1[q], el.hn), Eq = interp<NVC>(tab->N1[q], el.En),
                             nuq = interp<NVC>(tab->N1[q], el.nun);
                const TopStrain ts = top_strain<NPC, NVC>(*tab, q, g, el.hn, ewm, xe, hq);
                double sig[3];
                const double vm = von_mises(ts, Eq, nuq, sig);
                const double p = pow(ms * vm, rho);
                acc += wj * p;
                if (regc != 0.0) acc += wj * regc * pow(hq, rho);
                if (!GRAD) continue;
                if (regc != 0.0) {
                    const double dr = wj * regc * rho * pow(hq, rho - 1.0);
                    for (int b = 0; b < NVC; ++b) {
                        ge[b] += dr * (ewm ? 1.0 : tab->N1[q][b]);
                        if (ewm) break;
                    }
                }
                if (!(vm > 0.0)) continue;                      // zero stress: zero contribution (subgradient)
                const double dp = wj * rho * p / vm;            // d/dvm of wj (m vm)^rho
                double de[3];
                dvm_deps(sig, vm, Eq, nuq, de);
                // d/dw: through the strains, and through -1/2 b (x) gradx(h) with b0 = -theta.E1, b1 = theta.E0, theta = sum_b NR_b theta_b
                Gen t;
                const double z = 0.5 * hq;
                t.e00 = dp * de[0]; t.e11 = dp * de[1]; t.g01 = dp * de[2];
                t.k00 = -z * t.e00; t.k11 = -z * t.e11; t.k01 = -z * t.g01;
                t.ga0 = t.ga1 = t.om = 0.0;
                strains_T_q<NPC, NVC>(*tab, q, g, t, ye);
                const double cb0 = -0.5 * (t.e00 * ts.gh0 + t.g01 * ts.gh1), cb1 = -0.5 * (t.e11 * ts.gh1 + t.g01 * ts.gh0);
                for (int b = 0; b < NVC; ++b)
                    for (int c = 0; c < 3; ++c) ye[3 * NPC + 3 * b + c] += tab->NR[q][b] * (-cb0 * g.E1[c] + cb1 * g.E0[c]);
                // d/dh: z = h/2 and, for nodal thickness, gradx(h)
                for (int b = 0; b < NVC; ++b) {
                    const double Mb = ewm ? 1.0 : tab->N1[q][b];
                    double d0 = -0.5 * Mb * ts.k00, d1 = -0.5 * Mb * ts.k11, d2 = -0.5 * Mb * ts.k01;
                    if (!ewm) {
                        const double r0 = tab->dN1[q][b][0], r1 = tab->dN1[q][b][1];
                        const double m0 = r0 * g.Q[0][0] + r1 * g.Q[1][0], m1 = r0 * g.Q[0][1] + r1 * g.Q[1][1];
                        d0 -= 0.5 * ts.b0 * m0;
                        d1 -= 0.5 * ts.b1 * m1;
                        d2 -= 0.5 * (ts.b0 * m1 + ts.b1 * m0);
                    }
                    ge[b] += dp * (de[0] * d0 + de[1] * d1 + de[2] * d2);
                    if (ewm) break;
                }
            }
        }
        if (GRAD && pos < m.nel) {
            double* dst = ybuf + ((size_t)(l - l0) * m.nel + pos) * YSTRIDE;
            for (int i = 0; i < LD; ++i) dst[i] = act ? scale * ye[i] : 0.0;
        }
        block_sum_store(acc, bsum + (size_t)l * gridDim.x + blockIdx.x);
    }
    if (GRAD && pos < m.nel) {
        double* dst = tbuf + ((size_t)blockIdx.y * m.nel + e) * NVC;
        for (int b = 0; b < NVC; ++b) dst[b] = act ? scale * ge[b] : 0.0;
    }
}

// per_level[l] = sum over the blocks of bsum[l * nbx + .], in block order
__global__ void __launch_bounds__(256)
k_hist_level_sums(int levels, int nbx, const double* __restrict__ bsum, double* __restrict__ per_level) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= levels) return;
    double s = 0.0;
    for (int k = 0; k < nbx; ++k) s += bsum[(size_t)l * nbx + k];
    per_level[l] = s;
}

// acc[i] (+)= sum over the level groups of tbuf[g len + i], in group order
__global__ void __launch_bounds__(256)
k_hist_group_sum(int64_t len, int ngroups, int first, const double* __restrict__ tbuf, double* __restrict__ acc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    double s = first ? 0.0 : acc[i];
    for (int g = 0; g < ngroups; ++g) s += tbuf[(size_t)g * len + i];
    acc[i] = s;
}

// per-cell thickness: out[e] = acc[nvc e]
__global__ void __launch_bounds__(256)
k_hist_cell_pick(int nel, int nvc, const double* __restrict__ acc, double* __restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nel) out[e] = acc[(size_t)nvc * e];
}

// d P_l / d w of the levels of a chunk: k_gather_sum with grid.y over the levels (ybuf and out advance by one level each)
template <int NPC, int NVC>
__global__ void __launch_bounds__(256)
k_hist_gather(int nP2, int nV, int nel, int ndof_u, int ndof, const int* __restrict__ n2e_off, const int* __restrict__ n2e_ent,
              const double* __restrict__ ybuf, double* __restrict__ out, int cr, int nrot) {
    gather_sum_node<NPC, NVC>(blockIdx.x * blockDim.x + threadIdx.x, nP2, nV, ndof_u, ndof, n2e_off, n2e_ent,
                              ybuf + (size_t)blockIdx.y * nel * YSTRIDE, out + (size_t)blockIdx.y * ndof, cr, nrot);
}

}  // namespace femo
