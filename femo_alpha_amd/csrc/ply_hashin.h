// Hashin fibre and matrix failure indices of laminated shells (Hashin 1980, plane stress, his fibre-tension shear factor alpha = 0),
// aggregates and fields, gfx950, fp64.  Reads entries 0..9 (G, z) of the ply table of ply_failure.h and a strengths table of
// HSH_W = 6 doubles per (cell, recovery point): [Xt, Xc, Yt, Yc, SL, ST], all finite and > 0 (k_hashin_check).
//
// With sigma = (s1, s2, t12) = G (eps - z kappa) of ply_fi at quadrature point q of the degree-4 stress measure and recovery point p:
//   fibre   FI_f = (s1 / Xt)^2                                   s1 >= 0
//           FI_f = (s1 / Xc)^2                                   s1 <  0
//   matrix  FI_m = (s2 / Yt)^2 + (t12 / SL)^2                    s2 >= 0
//           FI_m = (s2 / (2 ST))^2 + c1 s2 + (t12 / SL)^2        s2 <  0,    c1 = ((Yc / (2 ST))^2 - 1) / Yc
// The formula switches on the sign of a stress component, which no table of quadratic forms can express.  FI_f is C1 and sqrt(FI_f)
// is proportional to the load; FI_m is continuous with a derivative kink at s2 = 0 unless ST = Yc / 2, may be negative, and is
// differentiated on the branch of the sign.  A zero takes the tension branch; a NaN passes through.
//   dFI_f / dsigma = (2 s1 / X^2, 0, 0)                          X the strength of the branch
//   dFI_m / dsigma = (0, 2 s2 / Yt^2, 2 t12 / SL^2)              tension
//   dFI_m / dsigma = (0, s2 / (2 ST^2) + c1, 2 t12 / SL^2)       compression
// G and z enter through sigma as in PF_DTABLE: outer(sbar, x) and -(G^T sbar) . kappa; columns 10..15 of the table gradient are
// exact zeros.  Derivatives with respect to the strengths are not provided.
//   S = log sum_e sum_q wj_q sum_p exp(rho FI_eqp),    K = (S - log(alpha npt)) / rho,    dK / dFI_eqp = wj_q exp(rho FI_eqp - S).
// The reference has no ply recovery: this is the project's own contract, pinned by tests/ply_hashin_ref.py.
//
// The layout is k_ply_failure's: one thread per cell, one wave per block; the six strains (and wj) of every quadrature point are
// formed once and parked in the thread's own column of LDS (rolled loop, no barrier: columns are private), come back into registers,
// and the recovery points stream through them, p outermost, so that every entry of the entry-major tables is read once.  The branch
// is chosen with selects on the sign: the lanes of a wave never diverge on it.  IDX: 0 fibre, 1 matrix; a kernel loads only the
// rows of G and the strengths its index reads.
//   PH_VALUE   running pairs (m, z) = (max u, sum wj exp(u - m)), u = rho FI; wave butterfly, one slot (m, z, reference area) per
//              block, merged in block order by k_ply_combine.  No atomics.
//   PH_FIELD   both indices in one pass over the strains: out[e npt + p] = max_q FI_f, out2[e npt + p] = max_q FI_m (either pointer
//              may be null; every cell, whatever the selected sub-domain); the first maximiser in quadrature order wins and a NaN
//              stays visible (the update of PF_FIELD).  IDX is not read.
//   PH_DW      strain cotangents per quadrature point first, then ONE strains_T_q per point; the element vector goes to the cell's
//              slot of ybuf for k_gather_sum (fixed order, no atomics)
//   PH_DTABLE  every cell writes its own 16 npt row (cell-major, the layout of the ply table's ABI); zeros outside the selection
// The gradient modes take a cotangent cbar (nel npt, cell-major) or null.  Null: the aggregate, coefficient wj_q exp(rho FI - S) at
// every q, S read from device memory (res[0] of k_ply_combine).  Given: the reverse mode of the field, coefficient cbar_ep at the
// first maximiser q* alone, every cell live.  What the derivative needs at q* travels with the maximum through selects over the
// unrolled q, as in ply_strength.h; the strain cotangents are then summed in the thread's LDS column at the run-time index q*.
// Nothing indexes a register array at run time.
#pragma once
#include "shell_device.h"
#include "stress_grad.h"
#include "ply_failure.h"
#include "ply_field_rev.h"
#include "ply_strength.h"

namespace femo {

constexpr int HSH_W = 6;           // strengths per recovery point: Xt, Xc, Yt, Yc, SL, ST
enum { PH_VALUE = 0, PH_FIELD = 1, PH_DW = 2, PH_DTABLE = 3 };
enum { PH_FIBRE = 0, PH_MATRIX = 1 };

// what index IDX reads of recovery point p of cell e: the rows R0 .. R1 - 1 of G, z, and the coefficients of its two branches
//   fibre   qt = 1 / Xt^2, qc = 1 / Xc^2
//   matrix  qt = 1 / Yt^2, qc = 1 / (2 ST)^2, c1, sl = 1 / SL^2
template <int IDX>
struct HashinPoint {
    static constexpr int R0 = IDX == PH_FIBRE ? 0 : 1, R1 = IDX == PH_FIBRE ? 1 : 3;
    double G[3][3], z, qt, qc, c1, sl;
};

template <int IDX>
__device__ __forceinline__ void load_hashin(const double* __restrict__ T, const double* __restrict__ H, int nel, int e, int p, HashinPoint<IDX>& P) {
    const double* s = T + (size_t)p * PLY_W * nel + e;
    const double* h = H + (size_t)p * HSH_W * nel + e;
#pragma unroll
    for (int i = HashinPoint<IDX>::R0; i < HashinPoint<IDX>::R1; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) P.G[i][j] = s[(size_t)(3 * i + j) * nel];
    P.z = s[(size_t)9 * nel];
    if constexpr (IDX == PH_FIBRE) {
        const double Xt = h[0], Xc = h[(size_t)nel];
        P.qt = 1.0 / (Xt * Xt);
        P.qc = 1.0 / (Xc * Xc);
        P.c1 = P.sl = 0.0;
    } else {
        const double Yt = h[(size_t)2 * nel], Yc = h[(size_t)3 * nel], SL = h[(size_t)4 * nel], ST = h[(size_t)5 * nel];
        const double r = Yc / (2.0 * ST);                    // exactly 1 at ST = Yc / 2: c1 is then an exact zero
        P.qt = 1.0 / (Yt * Yt);
        P.qc = 1.0 / (4.0 * ST * ST);
        P.c1 = (r * r - 1.0) / Yc;
        P.sl = 1.0 / (SL * SL);
    }
}

// s: (e00, e11, g01, k00, k11, k01) of the point; x = eps - z kappa; sig: the rows of sigma = G x the index reads; returns FI and the
// coefficients (a, b) of its branch: dFI / d s_d = 2 a s_d + b with d the component the sign is taken of
template <int IDX>
__device__ __forceinline__ double hashin_fi(const HashinPoint<IDX>& P, const double* s, double* x, double* sig, double& a, double& b) {
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = s[j] - P.z * s[3 + j];
#pragma unroll
    for (int i = HashinPoint<IDX>::R0; i < HashinPoint<IDX>::R1; ++i) sig[i] = P.G[i][0] * x[0] + P.G[i][1] * x[1] + P.G[i][2] * x[2];
    if constexpr (IDX == PH_FIBRE) {
        a = sig[0] >= 0.0 ? P.qt : P.qc;                     // a NaN takes the compression branch and passes through the square
        b = 0.0;
        return a * sig[0] * sig[0];
    } else {
        const bool t = sig[1] >= 0.0;
        a = t ? P.qt : P.qc;
        b = t ? 0.0 : P.c1;
        return a * sig[1] * sig[1] + b * sig[1] + P.sl * sig[2] * sig[2];
    }
}

// c dFI / dsigma, the rows the index reads
template <int IDX>
__device__ __forceinline__ void hashin_dfi(const HashinPoint<IDX>& P, const double* sig, double a, double b, double c, double* sb) {
    if constexpr (IDX == PH_FIBRE) {
        sb[0] = c * 2.0 * a * sig[0];
    } else {
        sb[1] = c * (2.0 * a * sig[1] + b);
        sb[2] = c * 2.0 * P.sl * sig[2];
    }
}

// t = G^T sbar over the rows of the index
template <int IDX>
__device__ __forceinline__ void hashin_GT(const HashinPoint<IDX>& P, const double* sb, double* t) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double v = 0.0;
#pragma unroll
        for (int i = HashinPoint<IDX>::R0; i < HashinPoint<IDX>::R1; ++i) v += P.G[i][j] * sb[i];
        t[j] = v;
    }
}

// acc (PLY_W) += c dFI / d(G, z) at one point (x = eps - z kappa, kap = kappa); the rows of G the index does not read and the
// columns 10..15 are never touched
template <int IDX>
__device__ __forceinline__ void hashin_dtable(const HashinPoint<IDX>& P, const double* sig, const double* x, const double* kap, double a, double b,
                                              double c, double* acc) {
    double sb[3], t[3];
    hashin_dfi<IDX>(P, sig, a, b, c, sb);
#pragma unroll
    for (int i = HashinPoint<IDX>::R0; i < HashinPoint<IDX>::R1; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[3 * i + j] += sb[i] * x[j];
    hashin_GT<IDX>(P, sb, t);
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[9] -= t[j] * kap[j];
}

// the maximiser q* of FI over the points' strains s (the update of PH_FIELD), with the branch coefficients, sigma, x and kappa at q*
template <int IDX, int NQ>
__device__ __forceinline__ int hashin_maximiser(const HashinPoint<IDX>& P, const double (&s)[NQ][6], double& am, double& bm, double* sigm, double* xm,
                                                double* km) {
    double mx = -INFINITY;
    int qs = 0;
    am = bm = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) sigm[j] = xm[j] = km[j] = 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double x[3], sig[3], a, b;
        const double fi = hashin_fi<IDX>(P, s[q], x, sig, a, b);
        const bool take = fi > mx || fi != fi;               // the first point in quadrature order wins; a NaN stays visible
        mx = take ? fi : mx;
        qs = take ? q : qs;
        am = take ? a : am;
        bm = take ? b : bm;
#pragma unroll
        for (int i = HashinPoint<IDX>::R0; i < HashinPoint<IDX>::R1; ++i) sigm[i] = take ? sig[i] : sigm[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            xm[j] = take ? x[j] : xm[j];
            km[j] = take ? s[q][3 + j] : km[j];
        }
    }
    return qs;
}

// res: shift S of the aggregate's gradient modes (read when cbar is null); cbar: cotangent of the field (nel npt) or null; eslot: slot
// of every cell in ybuf (PH_DW); out: part (PH_VALUE, 3 doubles per block), the fibre field (PH_FIELD), ybuf (PH_DW), d / d table
// (PH_DTABLE); out2: the matrix field (PH_FIELD).  m selects the sub-domain: the caller passes every cell with a cotangent.
template <int NPC, int NVC, bool QUAD, bool UHAT, int MODE, int IDX>
__global__ void __launch_bounds__(PLY_BLOCK)
k_ply_hashin(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const double* __restrict__ plyT, const double* __restrict__ hshT, int npt,
             double rho, const double* __restrict__ w, const double* __restrict__ res, const double* __restrict__ cbar,
             const int* __restrict__ eslot, double* __restrict__ out, double* __restrict__ out2) {
    constexpr int LD = 3 * NPC + 3 * NVC, NQ = QUAD ? 9 : 6;
    constexpr int ROWS = MODE == PH_FIELD ? 6 : 7;          // per quadrature point: the strains, and the weight where a mode needs it
    __shared__ double s_q[ROWS * NQ][PLY_BLOCK];
    const int tid = threadIdx.x, e = blockIdx.x * PLY_BLOCK + tid;
    const bool live = e < m.nel && (MODE == PH_FIELD || cell_selected(m, e));
    double km = -INFINITY, kz = 0.0, area = 0.0;
    if (live) {
        Elem<NPC, NVC> el;
        load_elem<NPC, NVC, UHAT>(m, f, e, el);
        double s[NQ][6], wj[NQ];
        if constexpr (MODE == PH_FIELD) ply_point_strains<NPC, NVC, QUAD, UHAT, NQ>(m, tab, el, w, s_q, tid, s);
        else area = ply_point_strains_w<NPC, NVC, QUAD, UHAT, NQ>(m, tab, el, w, s_q, tid, s, wj);
        if constexpr (MODE == PH_FIELD) {
            for (int p = 0; p < npt; ++p) {
                HashinPoint<PH_FIBRE> Pf;
                HashinPoint<PH_MATRIX> Pm;
                load_hashin<PH_FIBRE>(plyT, hshT, m.nel, e, p, Pf);
                load_hashin<PH_MATRIX>(plyT, hshT, m.nel, e, p, Pm);
                double mf = -INFINITY, mm = -INFINITY;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    double x[3], sig[3], a, b;
                    const double ff = hashin_fi<PH_FIBRE>(Pf, s[q], x, sig, a, b);
                    const double fm = hashin_fi<PH_MATRIX>(Pm, s[q], x, sig, a, b);
                    mf = ff > mf || ff != ff ? ff : mf;
                    mm = fm > mm || fm != fm ? fm : mm;
                }
                if (out) out[(size_t)e * npt + p] = mf;
                if (out2) out2[(size_t)e * npt + p] = mm;
            }
        } else if constexpr (MODE == PH_VALUE) {
            for (int p = 0; p < npt; ++p) {
                HashinPoint<IDX> P;
                load_hashin<IDX>(plyT, hshT, m.nel, e, p, P);
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    double x[3], sig[3], a, b;
                    ks_push_w(km, kz, rho * hashin_fi<IDX>(P, s[q], x, sig, a, b), wj[q]);
                }
            }
        } else if constexpr (MODE == PH_DW) {
            // the strains are in registers: the column now collects the strain cotangents per quadrature point
            if (cbar) {
                for (int i = 0; i < 7 * NQ; ++i) s_q[i][tid] = 0.0;
                const double* __restrict__ cb = cbar + (size_t)e * npt;
                for (int p = 0; p < npt; ++p) {
                    HashinPoint<IDX> P;
                    load_hashin<IDX>(plyT, hshT, m.nel, e, p, P);
                    double am, bm, sigm[3], xm[3], kpm[3], sb[3], t[3];
                    const int qs = hashin_maximiser<IDX, NQ>(P, s, am, bm, sigm, xm, kpm);
                    hashin_dfi<IDX>(P, sigm, am, bm, cb[p], sb);
                    hashin_GT<IDX>(P, sb, t);
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        s_q[7 * qs + j][tid] += t[j];
                        s_q[7 * qs + 3 + j][tid] -= P.z * t[j];
                    }
                }
            } else {
                const double sh = res[0];
                double eb[NQ][3], kb[NQ][3];
#pragma unroll
                for (int q = 0; q < NQ; ++q)
#pragma unroll
                    for (int j = 0; j < 3; ++j) eb[q][j] = kb[q][j] = 0.0;
                for (int p = 0; p < npt; ++p) {
                    HashinPoint<IDX> P;
                    load_hashin<IDX>(plyT, hshT, m.nel, e, p, P);
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        double x[3], sig[3], sb[3], t[3], a, b;
                        const double fi = hashin_fi<IDX>(P, s[q], x, sig, a, b);
                        hashin_dfi<IDX>(P, sig, a, b, wj[q] * exp(rho * fi - sh), sb);
                        hashin_GT<IDX>(P, sb, t);
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            eb[q][j] += t[j];
                            kb[q][j] -= P.z * t[j];
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < NQ; ++q)
#pragma unroll
                    for (int j = 0; j < 3; ++j) { s_q[7 * q + j][tid] = eb[q][j]; s_q[7 * q + 3 + j][tid] = kb[q][j]; }
            }
            ply_strain_cotangents_to_ybuf<NPC, NVC, QUAD, UHAT, NQ>(tab, el, s_q, tid, eslot, e, out);
        } else {
            const double sh = cbar ? 0.0 : res[0];
            for (int p = 0; p < npt; ++p) {
                HashinPoint<IDX> P;
                load_hashin<IDX>(plyT, hshT, m.nel, e, p, P);
                double acc[PLY_W];
#pragma unroll
                for (int k = 0; k < PLY_W; ++k) acc[k] = 0.0;
                if (cbar) {
                    double am, bm, sigm[3], xm[3], kpm[3];
                    hashin_maximiser<IDX, NQ>(P, s, am, bm, sigm, xm, kpm);
                    hashin_dtable<IDX>(P, sigm, xm, kpm, am, bm, cbar[(size_t)e * npt + p], acc);
                } else {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        double x[3], sig[3], a, b;
                        const double fi = hashin_fi<IDX>(P, s[q], x, sig, a, b);
                        hashin_dtable<IDX>(P, sig, x, &s[q][3], a, b, wj[q] * exp(rho * fi - sh), acc);
                    }
                }
                double* o = out + ((size_t)e * npt + p) * PLY_W;
#pragma unroll
                for (int k = 0; k < PLY_W; ++k) o[k] = acc[k];
            }
        }
    } else if (e < m.nel) {                      // outside the selected sub-domain
        if constexpr (MODE == PH_DW) ply_zero_ybuf_slot<LD>(eslot, e, out);
        else if constexpr (MODE == PH_DTABLE) ply_zero_table_row<PLY_W>(e, npt, out);
    }
    if constexpr (MODE == PH_VALUE) ply_block_slot(km, kz, area, tid, out);
}

// Every strength finite and > 0.  tab: the cell-major strengths table, n its entries.  *first (set to INT_MAX by the caller) receives
// the smallest offending flat index (e npt + p) 6 + k: an integer minimum, whose result does not depend on order.
__global__ void __launch_bounds__(256)
k_hashin_check(const double* __restrict__ tab, long long n, int* __restrict__ first) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = tab[i];
    const bool ok = v > 0.0 && v < INFINITY;                 // false for a NaN
    if (!ok) atomicMin(first, (int)i);
}

}  // namespace femo
