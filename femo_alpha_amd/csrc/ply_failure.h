// Ply failure aggregate and field of laminated shells (laminate mode, include/femo_hip.h: femo_set_ply_table), gfx950, fp64.
//
// Per cell npt recovery points of PLY_W = 16 doubles [G (3x3 row-major), z, F1, F2, F11, F22, F66, F12]:
//   sigma = (s1, s2, t12) = G (eps - z kappa)      eps, kappa: the Voigt membrane strains and curvatures of strains_q
//   FI    = F1 s1 + F2 s2 + F11 s1^2 + F22 s2^2 + F66 t12^2 + 2 F12 s1 s2
// at the points q of the degree-4 rule (Tables of the stress measure), weights wj_q = w_q det_q Ju_q, and
//   S = log sum_e sum_q wj_q sum_p exp(rho FI_eqp),    K = (S - log(alpha npt)) / rho,    dK / dFI_eqp = wj_q exp(rho FI_eqp - S).
// The reference has no ply recovery: this is the project's own contract, pinned by tests/ply_failure_ref.py.
//
// One thread per cell, one wave per block.  A pass over the quadrature points forms the geometry and the six strains of every point
// ONCE and parks them in the thread's own column of LDS (rolled loop, no barrier: columns are private); they come back into registers
// and the recovery points are then streamed through them, p outermost, so that every entry of the table is read exactly once.  The
// device copy of the table is entry-major ([16 p + k][nel], as xyz / cells are stored): the 64 cells of a wave read 512 contiguous
// bytes per entry.
//   PF_VALUE   running pairs (m, z) = (max u, sum wj exp(u - m)), u = rho FI: any finite u is safe.  Merged over the wave by a
//              butterfly, one slot (m, z, reference area) per block; k_ply_combine merges the slots in block order.  No atomics.
//   PF_FIELD   out[e npt + p] = max_q FI (every cell, whatever the selected sub-domain)
//   PF_DW      the cotangents of a point's strains, ebar = sum_p G^T sbar_p and kbar = sum_p -z_p G^T sbar_p, are summed over the
//              recovery points first; a second pass over the quadrature points (geometry again, once per point) pushes them through
//              ONE strains_T_q each.  The cell's element vector goes to its slot of ybuf for k_gather_sum (fixed order, no atomics).
//   PF_DTABLE  every cell writes its own 16 npt row of dK / d table (cell-major, the layout of the ABI); zeros outside the selection.
// The gradient kernels read the shift S from device memory (res[0] of k_ply_combine).
#pragma once
#include "shell_device.h"
#include "stress_grad.h"
#include "disp_history.h"

namespace femo {

constexpr int PLY_W = 16;          // doubles per recovery point
constexpr int PLY_MAX = 32;        // recovery points per cell
constexpr int PLY_BLOCK = 64;      // threads per block: one wave, 7 NQ columns of LDS (32 KB on quadrilaterals)
enum { PF_VALUE = 0, PF_FIELD = 1, PF_DW = 2, PF_DTABLE = 3 };

struct PlyPoint {
    double G[3][3], z, F1, F2, F11, F22, F66, F12;
};

// recovery point p of cell e from the entry-major device table
__device__ __forceinline__ void load_ply(const double* __restrict__ T, int nel, int e, int p, PlyPoint& P) {
    const double* s = T + (size_t)p * PLY_W * nel + e;
    double v[PLY_W];
#pragma unroll
    for (int k = 0; k < PLY_W; ++k) v[k] = s[(size_t)k * nel];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) P.G[i][j] = v[3 * i + j];
    P.z = v[9]; P.F1 = v[10]; P.F2 = v[11]; P.F11 = v[12]; P.F22 = v[13]; P.F66 = v[14]; P.F12 = v[15];
}

// s: (e00, e11, g01, k00, k11, k01) of the point; x = eps - z kappa, sig = G x; returns FI
__device__ __forceinline__ double ply_fi(const PlyPoint& P, const double* s, double* x, double* sig) {
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = s[j] - P.z * s[3 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) sig[i] = P.G[i][0] * x[0] + P.G[i][1] * x[1] + P.G[i][2] * x[2];
    return P.F1 * sig[0] + P.F2 * sig[1] + P.F11 * sig[0] * sig[0] + P.F22 * sig[1] * sig[1] + P.F66 * sig[2] * sig[2] +
           2.0 * P.F12 * sig[0] * sig[1];
}

// c dFI / d sigma
__device__ __forceinline__ void ply_dfi(const PlyPoint& P, const double* sig, double c, double* sb) {
    sb[0] = c * (P.F1 + 2.0 * (P.F11 * sig[0] + P.F12 * sig[1]));
    sb[1] = c * (P.F2 + 2.0 * (P.F22 * sig[1] + P.F12 * sig[0]));
    sb[2] = c * 2.0 * P.F66 * sig[2];
}

// one weighted entry into a running pair; m = -inf, z = 0 is the empty pair (d = +inf, e = 0: the entry replaces it)
__device__ __forceinline__ void ks_push_w(double& m, double& z, double u, double wt) {
    const double d = u - m;
    const double e = exp(-fabs(d));
    z = d > 0.0 ? z * e + wt : z + wt * e;
    m = d > 0.0 ? u : m;
}

// ---- device code shared by the kernels of all ply criteria (ply_failure.h, ply_shear.h, ply_strength.h, ply_hashin.h, ply_field_rev.h)

// the six strains of every degree-4 point of the state w, through the thread's column of LDS into registers
template <int NPC, int NVC, bool QUAD, bool UHAT, int NQ>
__device__ __forceinline__ void ply_point_strains(const MeshDev& m, const Tables* __restrict__ tab, const Elem<NPC, NVC>& el,
                                                  const double* __restrict__ w, double (*s_q)[PLY_BLOCK], int tid, double (&s)[NQ][6]) {
    constexpr int LD = 3 * NPC + 3 * NVC;
    {
        double xe[LD];
        load_state<NPC, NVC>(m, el, w, xe);
        for (int q = 0; q < NQ; ++q) {
            QPG g;
            qp_geometry<NVC, QUAD, UHAT>(el.X, el.Uh, tab->N1[q], tab->dN1[q], g);
            const Gen sq = strains_q<NPC, NVC>(*tab, q, g, xe);
            s_q[6 * q + 0][tid] = sq.e00; s_q[6 * q + 1][tid] = sq.e11; s_q[6 * q + 2][tid] = sq.g01;
            s_q[6 * q + 3][tid] = sq.k00; s_q[6 * q + 4][tid] = sq.k11; s_q[6 * q + 5][tid] = sq.k01;
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int k = 0; k < 6; ++k) s[q][k] = s_q[6 * q + k][tid];
}

// ply_point_strains with the weights: the six strains and wj_q = w_q det_q Ju_q of every degree-4 point through the thread's column
// of LDS (7 rows per point) into registers; returns the reference area sum_q w_q det_q
template <int NPC, int NVC, bool QUAD, bool UHAT, int NQ>
__device__ __forceinline__ double ply_point_strains_w(const MeshDev& m, const Tables* __restrict__ tab, const Elem<NPC, NVC>& el,
                                                      const double* __restrict__ w, double (*s_q)[PLY_BLOCK], int tid, double (&s)[NQ][6],
                                                      double (&wj)[NQ]) {
    constexpr int LD = 3 * NPC + 3 * NVC;
    double area = 0.0;
    {
        double xe[LD];
        load_state<NPC, NVC>(m, el, w, xe);
        for (int q = 0; q < NQ; ++q) {
            QPG g;
            qp_geometry<NVC, QUAD, UHAT>(el.X, el.Uh, tab->N1[q], tab->dN1[q], g);
            const Gen sq = strains_q<NPC, NVC>(*tab, q, g, xe);
            s_q[7 * q + 0][tid] = sq.e00; s_q[7 * q + 1][tid] = sq.e11; s_q[7 * q + 2][tid] = sq.g01;
            s_q[7 * q + 3][tid] = sq.k00; s_q[7 * q + 4][tid] = sq.k11; s_q[7 * q + 5][tid] = sq.k01;
            const double wd = tab->w[q] * g.det;
            s_q[7 * q + 6][tid] = wd * g.Ju;
            area += wd;                                  // alpha: area of the reference configuration, as for pnorm_stress
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s[q][k] = s_q[7 * q + k][tid];
        wj[q] = s_q[7 * q + 6][tid];
    }
    return area;
}

// The strain cotangents of every quadrature point, parked in the thread's column of LDS (7 rows per point, the first six: ebar,
// kbar), go through ONE strains_T_q each (geometry again, once per point); the cell's element vector goes to its slot of ybuf for
// k_gather_sum (fixed order, no atomics)
template <int NPC, int NVC, bool QUAD, bool UHAT, int NQ>
__device__ __forceinline__ void ply_strain_cotangents_to_ybuf(const Tables* __restrict__ tab, const Elem<NPC, NVC>& el, double (*s_q)[PLY_BLOCK],
                                                              int tid, const int* __restrict__ eslot, int e, double* __restrict__ out) {
    constexpr int LD = 3 * NPC + 3 * NVC;
    double ye[LD];
#pragma unroll
    for (int i = 0; i < LD; ++i) ye[i] = 0.0;
    for (int q = 0; q < NQ; ++q) {
        QPG g;
        qp_geometry<NVC, QUAD, UHAT>(el.X, el.Uh, tab->N1[q], tab->dN1[q], g);
        Gen tt;
        tt.e00 = s_q[7 * q + 0][tid]; tt.e11 = s_q[7 * q + 1][tid]; tt.g01 = s_q[7 * q + 2][tid];
        tt.k00 = s_q[7 * q + 3][tid]; tt.k11 = s_q[7 * q + 4][tid]; tt.k01 = s_q[7 * q + 5][tid];
        tt.ga0 = tt.ga1 = tt.om = 0.0;
        strains_T_q<NPC, NVC>(*tab, q, g, tt, ye);
    }
    double* dst = out + (size_t)eslot[e] * YSTRIDE;
#pragma unroll
    for (int i = 0; i < LD; ++i) dst[i] = ye[i];
}

// a cell outside the selected sub-domain: zeros in its slot of ybuf (the state gradients) ...
template <int LD>
__device__ __forceinline__ void ply_zero_ybuf_slot(const int* __restrict__ eslot, int e, double* __restrict__ out) {
    double* dst = out + (size_t)eslot[e] * YSTRIDE;
    for (int i = 0; i < LD; ++i) dst[i] = 0.0;
}

// ... and in its W npt row of the table gradient
template <int W>
__device__ __forceinline__ void ply_zero_table_row(int e, int npt, double* __restrict__ out) {
    double* o = out + (size_t)e * npt * W;
    for (int k = 0; k < npt * W; ++k) o[k] = 0.0;
}

// end of a value pass: the running pairs of the wave merged by a butterfly, the reference areas summed; lane 0 writes the block's slot
// (m, z, reference area) for k_ply_combine
__device__ __forceinline__ void ply_block_slot(double km, double kz, double area, int tid, double* __restrict__ out) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double m2 = shfl_xor_d(km, off), z2 = shfl_xor_d(kz, off);
        ks_merge(km, kz, m2, z2);
    }
    area = wave_sum(area);
    if (tid == 0) {
        double* p = out + (size_t)blockIdx.x * 3;
        p[0] = km; p[1] = kz; p[2] = area;
    }
}

// res: shift S of the gradient kernels (PF_DW, PF_DTABLE), read from device memory; eslot: slot of every cell in ybuf (PF_DW);
// out: part (PF_VALUE, 3 doubles per block), the field (PF_FIELD), ybuf (PF_DW), d K / d table (PF_DTABLE)
template <int NPC, int NVC, bool QUAD, bool UHAT, int MODE>
__global__ void __launch_bounds__(PLY_BLOCK)
k_ply_failure(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const double* __restrict__ plyT, int npt, double rho,
              const double* __restrict__ w, const double* __restrict__ res, const int* __restrict__ eslot, double* __restrict__ out) {
    constexpr int LD = 3 * NPC + 3 * NVC, NQ = QUAD ? 9 : 6;
    __shared__ double s_q[7 * NQ][PLY_BLOCK];
    const int tid = threadIdx.x, e = blockIdx.x * PLY_BLOCK + tid;
    const bool live = e < m.nel && (MODE == PF_FIELD || cell_selected(m, e));
    double km = -INFINITY, kz = 0.0, area = 0.0;
    if (live) {
        Elem<NPC, NVC> el;
        load_elem<NPC, NVC, UHAT>(m, f, e, el);
        double s[NQ][6], wj[NQ];
        area = ply_point_strains_w<NPC, NVC, QUAD, UHAT, NQ>(m, tab, el, w, s_q, tid, s, wj);
        if constexpr (MODE == PF_VALUE) {
            for (int p = 0; p < npt; ++p) {
                PlyPoint P;
                load_ply(plyT, m.nel, e, p, P);
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    double x[3], sig[3];
                    ks_push_w(km, kz, rho * ply_fi(P, s[q], x, sig), wj[q]);
                }
            }
        } else if constexpr (MODE == PF_FIELD) {
            for (int p = 0; p < npt; ++p) {
                PlyPoint P;
                load_ply(plyT, m.nel, e, p, P);
                double mx = -INFINITY;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    double x[3], sig[3];
                    const double fi = ply_fi(P, s[q], x, sig);
                    mx = fi > mx || fi != fi ? fi : mx;       // a NaN stays visible
                }
                out[(size_t)e * npt + p] = mx;
            }
        } else if constexpr (MODE == PF_DW) {
            const double sh = res[0];
            double eb[NQ][3], kb[NQ][3];
#pragma unroll
            for (int q = 0; q < NQ; ++q)
#pragma unroll
                for (int j = 0; j < 3; ++j) eb[q][j] = kb[q][j] = 0.0;
            for (int p = 0; p < npt; ++p) {
                PlyPoint P;
                load_ply(plyT, m.nel, e, p, P);
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    double x[3], sig[3], sb[3];
                    const double fi = ply_fi(P, s[q], x, sig);
                    ply_dfi(P, sig, wj[q] * exp(rho * fi - sh), sb);
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const double t = P.G[0][j] * sb[0] + P.G[1][j] * sb[1] + P.G[2][j] * sb[2];
                        eb[q][j] += t;
                        kb[q][j] -= P.z * t;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q)
#pragma unroll
                for (int j = 0; j < 3; ++j) { s_q[7 * q + j][tid] = eb[q][j]; s_q[7 * q + 3 + j][tid] = kb[q][j]; }
            ply_strain_cotangents_to_ybuf<NPC, NVC, QUAD, UHAT, NQ>(tab, el, s_q, tid, eslot, e, out);
        } else {
            const double sh = res[0];
            for (int p = 0; p < npt; ++p) {
                PlyPoint P;
                load_ply(plyT, m.nel, e, p, P);
                double a[PLY_W];
#pragma unroll
                for (int k = 0; k < PLY_W; ++k) a[k] = 0.0;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    double x[3], sig[3], sb[3];
                    const double fi = ply_fi(P, s[q], x, sig);
                    const double c = wj[q] * exp(rho * fi - sh);
                    ply_dfi(P, sig, c, sb);
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) a[3 * i + j] += sb[i] * x[j];
#pragma unroll
                    for (int j = 0; j < 3; ++j) a[9] -= (P.G[0][j] * sb[0] + P.G[1][j] * sb[1] + P.G[2][j] * sb[2]) * s[q][3 + j];
                    a[10] += c * sig[0];
                    a[11] += c * sig[1];
                    a[12] += c * sig[0] * sig[0];
                    a[13] += c * sig[1] * sig[1];
                    a[14] += c * sig[2] * sig[2];
                    a[15] += 2.0 * c * sig[0] * sig[1];
                }
                double* o = out + ((size_t)e * npt + p) * PLY_W;
#pragma unroll
                for (int k = 0; k < PLY_W; ++k) o[k] = a[k];
            }
        }
    } else if (e < m.nel) {                      // outside the selected sub-domain
        if constexpr (MODE == PF_DW) ply_zero_ybuf_slot<LD>(eslot, e, out);
        else if constexpr (MODE == PF_DTABLE) ply_zero_table_row<PLY_W>(e, npt, out);
    }
    if constexpr (MODE == PF_VALUE) ply_block_slot(km, kz, area, tid, out);
}

// res[0] = S = log sum wj exp(rho FI) (the shift of the gradient kernels), res[1] = reference area of the selection,
// res[2] = K = (S - log(alpha npt)) / rho with alpha = alpha_given if positive, else res[1]; res[3] = that alpha.
// The block slots are merged in block order: 256 contiguous runs, then the runs in order.
__global__ void __launch_bounds__(256)
k_ply_combine(int nb, const double* __restrict__ part, double alpha_given, int npt, double rho, double* __restrict__ res) {
    __shared__ double s_m[256], s_z[256], s_a[256];
    const int t = threadIdx.x, per = (nb + 255) / 256;
    double m = -INFINITY, z = 0.0, a = 0.0;
    for (int b = t * per; b < min(nb, (t + 1) * per); ++b) {
        ks_merge(m, z, part[3 * (size_t)b], part[3 * (size_t)b + 1]);
        a += part[3 * (size_t)b + 2];
    }
    s_m[t] = m; s_z[t] = z; s_a[t] = a;
    __syncthreads();
    if (t == 0) {
        for (int i = 1; i < 256; ++i) { ks_merge(m, z, s_m[i], s_z[i]); a += s_a[i]; }
        const double S = m + log(z), alpha = alpha_given > 0.0 ? alpha_given : a;
        res[0] = S;
        res[1] = a;
        res[2] = (S - log(alpha * npt)) / rho;
        res[3] = alpha;
    }
}

// device copy of the table: cell-major [e][16 p + k] (the ABI) -> entry-major [16 p + k][e]
__global__ void __launch_bounds__(256)
k_ply_transpose(const double* __restrict__ src, double* __restrict__ dst, int nel, int width) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)nel * width) return;
    const size_t e = i / width, k = i - e * width;
    dst[k * nel + e] = src[i];
}

}  // namespace femo
