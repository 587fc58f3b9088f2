// Reverse mode of the ply failure field (entry (e, p) = max_q FI_eqp, k_ply_failure<PF_FIELD>), gfx950, fp64.
//
// For a cotangent cbar (nel npt, cell-major like the field) the products (d field / d w)^T cbar and (d field / d table)^T cbar, and
// the partial Jacobians themselves.  The layout is that of the value kernel: one thread per cell, one wave per block, every cell
// whatever the selected sub-domain; the six strains of every degree-4 point are formed once, parked in the thread's own column of
// LDS (no barrier: columns are private) and come back into registers; the recovery points stream through them, p outermost, so that
// every entry of the entry-major table is read once.
//
// Maximiser: q* of a recovery point is found with the value kernel's own update (take = fi > mx || fi != fi, fi from the same ply_fi
// on the same strains): the first point in quadrature order wins and a NaN stays visible, so forward (k_ply_field_jvp) and reverse
// take the same branch even on ties.  What the derivative needs at q* (sigma, x, kappa) travels with the maximum through selects
// over the unrolled q; nothing indexes a register array at run time.
//
//   k_ply_field_vjp<.., false>  ybar_e = sum_p cbar_ep B_q*^T [G^T sbar; -z G^T sbar], sbar = dFI / dsigma.  The strain cotangents are
//                               summed per quadrature point first, in the thread's LDS column at the run-time index q* (the strains
//                               are in registers by then); one pass over the points then pushes them through ONE strains_T_q each,
//                               as PF_DW does.  The element vector goes to the cell's slot of ybuf for k_gather_sum: fixed order, no
//                               float atomics.
//   k_ply_field_vjp<.., true>   every cell writes its own 16 npt row, cell-major (the ABI layout of PF_DTABLE and of the layup's
//                               pull-back): the row of p is cbar_ep dFI / d(G, z, F.) at q* -- the expressions of PF_DTABLE with
//                               c = cbar_ep at one point.  Plain stores, every entry written.
//   k_ply_field_jac             row e npt + p: the LD entries of B_q*^T [G^T sbar; -z G^T sbar] with the global columns in the cell's
//                               local order (the convention of k_field_jac), or the 16 entries dFI / d(G, z, F.) at the columns
//                               16 (e npt + p) + k.  Rows do not overlap: plain stores.
#pragma once
#include "shell_device.h"
#include "stress_grad.h"
#include "ply_failure.h"

namespace femo {

// the maximiser q* of recovery point P over the points' strains s, with sigma, x = eps - z kappa and kappa at q*
template <int NQ>
__device__ __forceinline__ int ply_maximiser(const PlyPoint& P, const double (&s)[NQ][6], double* sigm, double* xm, double* km) {
    double mx = -INFINITY;
    int qs = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) sigm[j] = xm[j] = km[j] = 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double x[3], sig[3];
        const double fi = ply_fi(P, s[q], x, sig);
        const bool take = fi > mx || fi != fi;              // the value kernel's update: a NaN stays visible
        mx = take ? fi : mx;
        qs = take ? q : qs;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            sigm[j] = take ? sig[j] : sigm[j];
            xm[j] = take ? x[j] : xm[j];
            km[j] = take ? s[q][3 + j] : km[j];
        }
    }
    return qs;
}

// c dFI / d(G, z, F1, F2, F11, F22, F66, F12) at one point: the expressions of PF_DTABLE
__device__ __forceinline__ void ply_dfi_dtable(const PlyPoint& P, const double* sig, const double* x, const double* kap, double c, double* a) {
    double sb[3];
    ply_dfi(P, sig, c, sb);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) a[3 * i + j] = sb[i] * x[j];
    a[9] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) a[9] -= (P.G[0][j] * sb[0] + P.G[1][j] * sb[1] + P.G[2][j] * sb[2]) * kap[j];
    a[10] = c * sig[0];
    a[11] = c * sig[1];
    a[12] = c * sig[0] * sig[0];
    a[13] = c * sig[1] * sig[1];
    a[14] = c * sig[2] * sig[2];
    a[15] = 2.0 * c * sig[0] * sig[1];
}

// cbar: one cotangent, nel npt entries.  TABLE = false: out is ybuf (slot eslot[e], YSTRIDE doubles); TABLE = true: out is the
// cell-major table cotangent (16 npt nel), eslot unused.
template <int NPC, int NVC, bool QUAD, bool UHAT, bool TABLE>
__global__ void __launch_bounds__(PLY_BLOCK)
k_ply_field_vjp(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const double* __restrict__ plyT, int npt, const double* __restrict__ w,
                const double* __restrict__ cbar, const int* __restrict__ eslot, double* __restrict__ out) {
    constexpr int LD = 3 * NPC + 3 * NVC, NQ = QUAD ? 9 : 6;
    __shared__ double s_q[6 * NQ][PLY_BLOCK];
    const int tid = threadIdx.x, e = blockIdx.x * PLY_BLOCK + tid;
    if (e >= m.nel) return;
    Elem<NPC, NVC> el;
    load_elem<NPC, NVC, UHAT>(m, f, e, el);
    double s[NQ][6];
    ply_point_strains<NPC, NVC, QUAD, UHAT, NQ>(m, tab, el, w, s_q, tid, s);
    const double* __restrict__ cb = cbar + (size_t)e * npt;
    if constexpr (TABLE) {
        for (int p = 0; p < npt; ++p) {
            PlyPoint P;
            load_ply(plyT, m.nel, e, p, P);
            double sigm[3], xm[3], km[3], a[PLY_W];
            ply_maximiser<NQ>(P, s, sigm, xm, km);
            ply_dfi_dtable(P, sigm, xm, km, cb[p], a);
            double* o = out + ((size_t)e * npt + p) * PLY_W;
#pragma unroll
            for (int k = 0; k < PLY_W; ++k) o[k] = a[k];
        }
    } else {
        // the strains are in registers: the column now collects the strain cotangents per quadrature point
        for (int i = 0; i < 6 * NQ; ++i) s_q[i][tid] = 0.0;
        for (int p = 0; p < npt; ++p) {
            PlyPoint P;
            load_ply(plyT, m.nel, e, p, P);
            double sigm[3], xm[3], km[3], sb[3];
            const int qs = ply_maximiser<NQ>(P, s, sigm, xm, km);
            ply_dfi(P, sigm, cb[p], sb);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double t = P.G[0][j] * sb[0] + P.G[1][j] * sb[1] + P.G[2][j] * sb[2];
                s_q[6 * qs + j][tid] += t;
                s_q[6 * qs + 3 + j][tid] -= P.z * t;
            }
        }
        // ply_strain_cotangents_to_ybuf (ply_failure.h) written out: through the helper two instantiations of this kernel change their
        // register count
        double ye[LD];
#pragma unroll
        for (int i = 0; i < LD; ++i) ye[i] = 0.0;
        for (int q = 0; q < NQ; ++q) {
            QPG g;
            qp_geometry<NVC, QUAD, UHAT>(el.X, el.Uh, tab->N1[q], tab->dN1[q], g);
            Gen tt;
            tt.e00 = s_q[6 * q + 0][tid]; tt.e11 = s_q[6 * q + 1][tid]; tt.g01 = s_q[6 * q + 2][tid];
            tt.k00 = s_q[6 * q + 3][tid]; tt.k11 = s_q[6 * q + 4][tid]; tt.k01 = s_q[6 * q + 5][tid];
            tt.ga0 = tt.ga1 = tt.om = 0.0;
            strains_T_q<NPC, NVC>(*tab, q, g, tt, ye);
        }
        double* dst = out + (size_t)eslot[e] * YSTRIDE;
#pragma unroll
        for (int i = 0; i < LD; ++i) dst[i] = ye[i];
    }
}

// Partial Jacobian, one thread per cell looping over p.  TABLE = false: LD entries per row; TABLE = true: 16 entries per row.
template <int NPC, int NVC, bool QUAD, bool UHAT, bool TABLE>
__global__ void __launch_bounds__(PLY_BLOCK)
k_ply_field_jac(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const double* __restrict__ plyT, int npt, const double* __restrict__ w,
                double* __restrict__ vals, int* __restrict__ colidx) {
    constexpr int LD = 3 * NPC + 3 * NVC, NQ = QUAD ? 9 : 6;
    __shared__ double s_q[6 * NQ][PLY_BLOCK];
    const int tid = threadIdx.x, e = blockIdx.x * PLY_BLOCK + tid;
    if (e >= m.nel) return;
    Elem<NPC, NVC> el;
    load_elem<NPC, NVC, UHAT>(m, f, e, el);
    double s[NQ][6];
    ply_point_strains<NPC, NVC, QUAD, UHAT, NQ>(m, tab, el, w, s_q, tid, s);
    for (int p = 0; p < npt; ++p) {
        PlyPoint P;
        load_ply(plyT, m.nel, e, p, P);
        double sigm[3], xm[3], km[3];
        const int qs = ply_maximiser<NQ>(P, s, sigm, xm, km);
        const size_t r = (size_t)e * npt + p;
        if constexpr (TABLE) {
            double a[PLY_W];
            ply_dfi_dtable(P, sigm, xm, km, 1.0, a);
#pragma unroll
            for (int k = 0; k < PLY_W; ++k) {
                vals[r * PLY_W + k] = a[k];
                colidx[r * PLY_W + k] = (int)(r * PLY_W + k);
            }
        } else {
            double sb[3], t[3], ye[LD];
            ply_dfi(P, sigm, 1.0, sb);
#pragma unroll
            for (int j = 0; j < 3; ++j) t[j] = P.G[0][j] * sb[0] + P.G[1][j] * sb[1] + P.G[2][j] * sb[2];
            Gen tt;
            tt.e00 = t[0]; tt.e11 = t[1]; tt.g01 = t[2];
            tt.k00 = -P.z * t[0]; tt.k11 = -P.z * t[1]; tt.k01 = -P.z * t[2];
            tt.ga0 = tt.ga1 = tt.om = 0.0;
#pragma unroll
            for (int i = 0; i < LD; ++i) ye[i] = 0.0;
            QPG g;
            qp_geometry<NVC, QUAD, UHAT>(el.X, el.Uh, tab->N1[qs], tab->dN1[qs], g);
            strains_T_q<NPC, NVC>(*tab, qs, g, tt, ye);
            double* v = vals + r * LD;
            int* ci = colidx + r * LD;
#pragma unroll
            for (int a = 0; a < NPC; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) { v[3 * a + c] = ye[3 * a + c]; ci[3 * a + c] = 3 * el.pid[a] + c; }
#pragma unroll
            for (int b = 0; b < NVC; ++b)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    v[3 * NPC + 3 * b + c] = ye[3 * NPC + 3 * b + c];
                    ci[3 * NPC + 3 * b + c] = m.ndof_u + 3 * rot_node(m, el, b) + c;
                }
        }
    }
}

}  // namespace femo
