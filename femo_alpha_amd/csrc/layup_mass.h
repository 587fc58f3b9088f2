// Mass and volume of a laminate from its layup (include/femo_hip.h: femo_set_layup_density), gfx950, fp64.
//
// Over the selected sub-domain (femo_select_subdomain), on the quadrature tables "mass" uses (the full rule):
//   layup_mass   = sum_e (sum_k rho_k t_ek) W_e        layup_volume = sum_e (sum_k t_ek) W_e        W_e = sum_q w_q det_q J_q(uhat)
// The outputs see the layup directly, not through the laminate: d / d t_ek = rho_k W_e (or W_e), nothing depends on the angles, the state,
// the laminate or the table, and the shape derivative is the areal sum times d W_e / d uhat.
//
// The conventions of layup.h: one thread per cell, one wave per block, ply-major reads of t (512 contiguous bytes per ply and wave), the
// per-ply densities through the scalar path, the cell-major gradient out through the block's LDS slab.
//   k_layup_mass_value    both sums in one pass: wave_sum, one slot pair per block; k_layup_mass_combine merges the slots in block order.
//   k_layup_mass_dt       every cell writes its own nply row (zeros outside the selection).
// Neither uses an atomic: two identical calls return the same bits.  That promise covers the value and the thickness gradient only:
//   k_layup_mass_shape    dual arithmetic as in shape_sens.h, one thread per (cell, uhat component); the vertex accumulation uses the
//                         atomics of the other outputs' shape derivatives, so its last bits depend on the arrival order.
#pragma once
#include "layup.h"
#include "shape_sens.h"

namespace femo {

// W_e = sum_q w_q det_q J_q(uhat) of cell e
template <int NVC, bool QUAD, bool UHAT>
__device__ __forceinline__ double lm_cell_measure(const MeshDev& m, const FieldsDev& f, const Tables* __restrict__ tab, int e) {
    double X[NVC][3], Uh[NVC][3];
#pragma unroll
    for (int b = 0; b < NVC; ++b) {
        const int v = m.cells[b * m.nel + e];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            X[b][c] = m.xyz[3 * v + c];
            Uh[b][c] = UHAT ? f.uhat[3 * v + c] : 0.0;
        }
    }
    double W = 0.0;
    const int nq = tab->nq;
    for (int q = 0; q < nq; ++q) {
        QPG g;
        qp_geometry<NVC, QUAD, UHAT>(X, Uh, tab->N1[q], tab->dN1[q], g);
        W += tab->w[q] * g.det * g.Ju;
    }
    return W;
}

// part[2 b] = the block's share of layup_mass (0 without densities: rho null), part[2 b + 1] = its share of layup_volume
template <int NPC, int NVC, bool QUAD, bool UHAT>
__global__ void __launch_bounds__(LAY_BLOCK)
k_layup_mass_value(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const double* __restrict__ t, const double* __restrict__ rho, int nply,
                   double* __restrict__ part) {
    const int e = blockIdx.x * LAY_BLOCK + threadIdx.x;
    const size_t nel = (size_t)m.nel;
    double ms = 0.0, vs = 0.0;
    if (e < m.nel && cell_selected(m, e)) {
        const double W = lm_cell_measure<NVC, QUAD, UHAT>(m, f, tab, e);
        double H = 0.0, M = 0.0;
        for (int k = 0; k < nply; ++k) {
            const double tk = t[k * nel + e];
            H += tk;
            if (rho) M += rho[k] * tk;
        }
        ms = M * W;
        vs = H * W;
    }
    ms = wave_sum(ms);
    vs = wave_sum(vs);
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = ms;
        part[2 * (size_t)blockIdx.x + 1] = vs;
    }
}

// res[0] = layup_mass, res[1] = layup_volume: the block slots merged in block order, 256 contiguous runs, then the runs in order
__global__ void __launch_bounds__(256)
k_layup_mass_combine(int nb, const double* __restrict__ part, double* __restrict__ res) {
    __shared__ double s_m[256], s_v[256];
    const int t = threadIdx.x, per = (nb + 255) / 256;
    double ms = 0.0, vs = 0.0;
    for (int b = t * per; b < min(nb, (t + 1) * per); ++b) {
        ms += part[2 * (size_t)b];
        vs += part[2 * (size_t)b + 1];
    }
    s_m[t] = ms; s_v[t] = vs;
    __syncthreads();
    if (t == 0) {
        for (int i = 1; i < 256; ++i) { ms += s_m[i]; vs += s_v[i]; }
        res[0] = ms;
        res[1] = vs;
    }
}

// out (nel nply, cell-major) = d layup_mass / d t (rho: the nply densities) or d layup_volume / d t (rho null)
template <int NPC, int NVC, bool QUAD, bool UHAT>
__global__ void __launch_bounds__(LAY_BLOCK)
k_layup_mass_dt(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const double* __restrict__ rho, int nply, double* __restrict__ out) {
    __shared__ double sh[LAY_BLOCK * LAY_LD];
    const int e = blockIdx.x * LAY_BLOCK + threadIdx.x;
    if (e < m.nel) {
        const double W = cell_selected(m, e) ? lm_cell_measure<NVC, QUAD, UHAT>(m, f, tab, e) : 0.0;
        double* r = sh + threadIdx.x * LAY_LD;
        for (int k = 0; k < nply; ++k) r[k] = rho ? rho[k] * W : W;
    }
    __syncthreads();
    lay_slab_out(sh, out, m.nel, nply);
}

// out (3 nn) += (sum_k rho_k t_ek, or sum_k t_ek with rho null) d W_e / d uhat over the selected cells
template <int NVC, bool QUAD>
__global__ void __launch_bounds__(128)
k_layup_mass_shape(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const double* __restrict__ t, const double* __restrict__ rho, int nply,
                   double* __restrict__ out) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = gid / (3 * NVC), dir = gid - e * (3 * NVC);
    if (e >= m.nel || !cell_selected(m, e)) return;
    const int bseed = dir / 3, iseed = dir - 3 * bseed;
    const size_t nel = (size_t)m.nel;
    double X[NVC][3];
    D1 Uh[NVC][3];
    int vid[NVC];
    for (int b = 0; b < NVC; ++b) {
        const int v = m.cells[b * m.nel + e];
        vid[b] = v;
        for (int c = 0; c < 3; ++c) {
            X[b][c] = m.xyz[3 * v + c];
            Uh[b][c] = mk(f.uhat[3 * v + c], (b == bseed && c == iseed) ? 1.0 : 0.0);
        }
    }
    double areal = 0.0;
    for (int k = 0; k < nply; ++k) areal += (rho ? rho[k] : 1.0) * t[k * nel + e];
    D1 W = mk(0.0);
    const int nq = tab->nq;
    for (int q = 0; q < nq; ++q) {
        QPG g;
        double zero[NVC][3] = {};
        qp_geometry<NVC, QUAD, false>(X, zero, tab->N1[q], tab->dN1[q], g);
        QPD s;
        qp_shape_dual<NVC, QUAD>(X, Uh, tab->dN1[q], g, s);
        W = W + (tab->w[q] * g.det) * s.Ju;
    }
    atomicAdd(&out[3 * vid[bseed] + iseed], areal * W.d);
}

}  // namespace femo
