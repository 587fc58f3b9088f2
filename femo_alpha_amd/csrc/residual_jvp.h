// Forward mode of the static residual: out = (dR/d arg) v at the stored state, gfx950, fp64.
//
// The reference assembles dR/d arg and multiplies (assembleMatrix + computeMatVecProductFwd, csdl_alpha_opt/state_operation.py:159-171,
// fea/utils_dolfinx.py:275-283).  Here no matrix is formed: every cell evaluates the directional derivative of its own residual and
// parks the 3 NPC + 3 NVC results in its slot of the element-result buffer, which k_gather_sum adds up per node -- the two passes of
// the operator itself (k_apply4), so there are no float atomics and the summation order is fixed: two calls return the same bits.
//
// One kernel, one structure (that of k_apply4: four lanes of a DPP quad per cell, each a quarter of the quadrature points, the cell's
// nodal data staged in LDS, partial results combined with quad_xor_sum), with the point's work chosen by MODE:
//   JVP_H / JVP_E / JVP_NU   y_e = sum_q B^T (dC/d field . dfield(q)) B w      (dfield interpolated as the field is)
//   JVP_LAM                  y_e = sum_q B^T C[sym dir_e] B w                  (R is linear in the laminate values)
//   JVP_LOAD                 y_e = - int N_a df J dx
//   JVP_SHAPE(_LAM)          y_e = d/d eps R_e(w; uhat + eps dir): forward-mode duals through the geometry (shape_sens.h), the cell's
//                            nodal uhat carrying the direction as its dual part -- one pass per direction per cell
#pragma once
#include "shape_sens.h"

namespace femo {

enum { JVP_H = DERIV_H, JVP_E = DERIV_E, JVP_NU = DERIV_NU, JVP_LAM = 4, JVP_LOAD = 5, JVP_SHAPE = 6, JVP_SHAPE_LAM = 7 };

// the conjugate stresses as duals; J(uhat) multiplies shear and drilling only (linear_shell_model.py:275-296)
template <bool LAM>
__device__ __forceinline__ GenD stress_dual(const GenD& s, double h, double E, double nu, const double* L, double hK, double wdetS,
                                            double wdet, D1 Ju) {
    GenD t;
    if constexpr (LAM) {
        auto A = [&](int blk, int i, int j) { return L[9 * blk + 3 * i + j]; };
        const D1 ep[3] = {s.e00, s.e11, s.g01}, kp[3] = {s.k00, s.k11, s.k01};
        D1 n[3], mo[3];
        for (int i = 0; i < 3; ++i) {
            n[i] = mk(0.0); mo[i] = mk(0.0);
            for (int j = 0; j < 3; ++j) {
                const double b = A(1, i, j);
                n[i] = n[i] + A(0, i, j) * ep[j] + b * kp[j];
                mo[i] = mo[i] + b * ep[j] + A(2, i, j) * kp[j];
            }
        }
        t.e00 = wdetS * n[0]; t.e11 = wdetS * n[1]; t.g01 = wdetS * n[2];
        t.k00 = wdetS * mo[0]; t.k11 = wdetS * mo[1]; t.k01 = wdetS * mo[2];
        const D1 cs = wdetS * Ju;
        t.ga0 = cs * (L[27] * s.ga0 + L[28] * s.ga1);
        t.ga1 = cs * (L[28] * s.ga0 + L[30] * s.ga1);
        t.om = ((wdet * L[31] / (hK * hK)) * Ju) * s.om;
    } else {
        const double c = E / (1.0 - nu * nu), sh = 0.5 * (1.0 - nu);
        const double cm = c * h * wdetS, cb = c * h * h * h / 12.0 * wdetS;
        const D1 cs = (K_SHEAR * E / (2.0 * (1.0 + nu)) * h * wdetS) * Ju;
        const D1 cd = (E * h * h * h / (hK * hK) * wdet) * Ju;
        t.e00 = cm * (s.e00 + nu * s.e11);
        t.e11 = cm * (nu * s.e00 + s.e11);
        t.g01 = (cm * sh) * s.g01;
        t.k00 = cb * (s.k00 + nu * s.k11);
        t.k11 = cb * (nu * s.k00 + s.k11);
        t.k01 = (cb * sh) * s.k01;
        t.ga0 = cs * s.ga0;
        t.ga1 = cs * s.ga1;
        t.om = cd * s.om;
    }
    return t;
}

// yd += dual part of B^T t  (strains_T_q with the uhat-dependent geometry as duals)
template <int NPC, int NVC>
__device__ __forceinline__ void strains_T_dual(const Tables& t, int q, const QPG& g, const QPD& s, const GenD& tt, double* yd) {
    D1 H0[3], H1[3];
    const D1 a10 = tt.g01 - 0.5 * tt.om, a01 = tt.g01 + 0.5 * tt.om;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        H0[c] = g.E0[c] * tt.e00 + g.E1[c] * a10 + g.E2[c] * tt.ga0;
        H1[c] = g.E0[c] * a01 + g.E1[c] * tt.e11 + g.E2[c] * tt.ga1;
    }
#pragma unroll
    for (int a = 0; a < NPC; ++a) {
        const double r0 = t.dN2[q][a][0], r1 = t.dN2[q][a][1];
        const D1 d0 = r0 * s.Q[0][0] + r1 * s.Q[1][0], d1 = r0 * s.Q[0][1] + r1 * s.Q[1][1];
#pragma unroll
        for (int c = 0; c < 3; ++c) yd[3 * a + c] += (d0 * H0[c] + d1 * H1[c]).d;
    }
    D1 x00[3], x01[3], x10[3], x11[3];
    dcross(g.E0, s.w0, x00);
    dcross(g.E0, s.w1, x01);
    dcross(g.E1, s.w0, x10);
    dcross(g.E1, s.w1, x11);
    D1 Tq[3], C0[3], C1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Tq[c] = g.E1[c] * tt.ga0 - g.E0[c] * tt.ga1 + g.E2[c] * tt.om + tt.k00 * x00[c] + tt.k11 * x11[c] + tt.k01 * (x01[c] + x10[c]);
        C0[c] = g.E0[c] * tt.k01 - g.E1[c] * tt.k00;
        C1[c] = g.E0[c] * tt.k11 - g.E1[c] * tt.k01;
    }
#pragma unroll
    for (int b = 0; b < NVC; ++b) {
        const double r0 = t.dNR[q][b][0], r1 = t.dNR[q][b][1];
        const D1 m0 = r0 * s.Q[0][0] + r1 * s.Q[1][0], m1 = r0 * s.Q[0][1] + r1 * s.Q[1][1];
        const double Mb = t.NR[q][b];
#pragma unroll
        for (int c = 0; c < 3; ++c) yd[3 * NPC + 3 * b + c] += (Mb * Tq[c] + m0 * C0[c] + m1 * C1[c]).d;
    }
}

__global__ void k_negate(double* __restrict__ a, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) a[i] = -a[i];
}

constexpr int JVP_EPB = 64;     // cells per block of four waves (four lanes each)

// x: the state with its strong rows zeroed (what the residual's operator sees); dir: the direction in the argument's own layout;
// ybuf: slot `pos` (the cell's place in eorder) receives the cell's results
template <int NPC, int NVC, bool QUAD, bool UHAT, int MODE>
__global__ void __launch_bounds__(256, 2)
k_residual_jvp(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const int* __restrict__ eorder, const double* __restrict__ x,
               const double* __restrict__ dir, double* __restrict__ ybuf) {
    constexpr int LD = 3 * NPC + 3 * NVC;
    constexpr bool FIELD = MODE == JVP_H || MODE == JVP_E || MODE == JVP_NU;
    constexpr bool SHAPE = MODE == JVP_SHAPE || MODE == JVP_SHAPE_LAM;
    constexpr bool LAMLAW = MODE == JVP_LAM || MODE == JVP_SHAPE_LAM;
    constexpr bool STATE = MODE != JVP_LOAD;                    // the load term does not read the state
    constexpr int ODIR = 9 * NVC;                               // X, uhat, (h, E, nu) come first
    constexpr int OF = ODIR + (FIELD ? NVC : 3 * NVC);          // SHAPE: the nodal load behind the direction
    constexpr int GEO = OF + (SHAPE ? 3 * NVC : 0);
    __shared__ double sx[STATE ? JVP_EPB : 1][STATE ? LD + 1 : 1];
    __shared__ double sg[JVP_EPB][GEO + 1];
    __shared__ double slam[LAMLAW ? JVP_EPB : 1][LAMLAW ? LAM_W + 1 : 1];
    __shared__ Tables stab;
    {
        const double* src = reinterpret_cast<const double*>(tab);
        double* dst = reinterpret_cast<double*>(&stab);
        for (int i = threadIdx.x; i < (int)(sizeof(Tables) / sizeof(double)); i += blockDim.x) dst[i] = src[i];
    }
    const int lb = xcd_block(blockIdx.x, gridDim.x);
    const int le = threadIdx.x >> 2, sub = threadIdx.x & 3;
    const int pos = lb * JVP_EPB + le;
    const bool active = pos < m.nel;
    const int e = active ? (eorder ? eorder[pos] : pos) : 0;
    double hK = 0.0;
    if (active) {
        hK = m.hK[e];
        int pid[NPC], vid[NVC];
#pragma unroll
        for (int b = 0; b < NVC; ++b) vid[b] = m.cells[b * m.nel + e];
#pragma unroll
        for (int a = 0; a < NPC; ++a) pid[a] = m.cellp2[a * m.nel + e];
#pragma unroll
        for (int b = 0; b < NVC; ++b) {
            if (b == sub) {
                const int v = vid[b];
                const int tq = f.ewm ? e : v;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    sg[le][3 * b + c] = m.xyz[3 * v + c];
                    sg[le][3 * NVC + 3 * b + c] = (UHAT || SHAPE) ? f.uhat[3 * v + c] : 0.0;
                }
                sg[le][6 * NVC + b] = f.h[tq];
                sg[le][7 * NVC + b] = f.E[tq];
                sg[le][8 * NVC + b] = f.nu[tq];
                if constexpr (FIELD) sg[le][ODIR + b] = dir[tq];
                if constexpr (SHAPE) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        sg[le][ODIR + 3 * b + c] = dir[3 * v + c];
                        sg[le][OF + 3 * b + c] = f.f[3 * (f.ewp ? e : v) + c];
                    }
                }
                if constexpr (MODE == JVP_LOAD) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) sg[le][ODIR + 3 * b + c] = dir[3 * (f.ewp ? e : v) + c];
                }
            }
        }
        if constexpr (STATE) {
#pragma unroll
            for (int i = 0; i < LD; ++i) {
                if ((i % 4) == sub) {
                    const int node = i / 3, c = i - 3 * node;
                    const int rb = node >= NPC ? node - NPC : 0;
                    const int rnode = (NPC == 6 && NVC == 3 && m.cr) ? pid[(NVC + rb) % NPC] - m.nn : vid[rb];     // CG2CR1: the edge midpoint
                    const int g = node < NPC ? 3 * pid[node < NPC ? node : 0] + c : m.ndof_u + 3 * rnode + c;
                    sx[le][i] = x[g];
                }
            }
        }
        if constexpr (MODE == JVP_SHAPE_LAM) {
            const double* L = f.clt + (size_t)LAM_W * e;
#pragma unroll
            for (int k = 0; k < LAM_W; ++k)
                if ((k % 4) == sub) slam[le][k] = L[k];
        }
        if constexpr (MODE == JVP_LAM) {
            // the law acts through the symmetric parts of its blocks (femo_set_laminate), so the direction does too
            const double* L = dir + (size_t)LAM_W * e;
#pragma unroll
            for (int k = 0; k < LAM_W; ++k) {
                if ((k % 4) == sub) {
                    int kt = k;                                  // the transposed entry inside the block
                    if (k < 27) { const int blk = k / 9, r = k - 9 * blk, i = r / 3, j = r - 3 * i; kt = 9 * blk + 3 * j + i; }
                    else if (k == 28) kt = 29;
                    else if (k == 29) kt = 28;
                    slam[le][k] = 0.5 * (L[k] + L[kt]);
                }
            }
        }
    }
    __syncthreads();
    if (!active) return;
    double ye[LD];
#pragma unroll
    for (int i = 0; i < LD; ++i) ye[i] = 0.0;
    const int nq = stab.nq;
    for (int q = sub; q < nq; q += 4) {
        // re-derive the LDS rows every iteration (as k_apply4 does): keeps the staged values out of registers
        int row = le;
        asm volatile("" : "+v"(row));
        const double* xe = sx[STATE ? row : 0];
        const double* ge = sg[row];
        const double (*X)[3] = reinterpret_cast<const double (*)[3]>(ge);
        QPG g;
        if constexpr (SHAPE) {
            D1 Uh[NVC][3];
            double zero[NVC][3] = {};
#pragma unroll
            for (int b = 0; b < NVC; ++b)
#pragma unroll
                for (int c = 0; c < 3; ++c) Uh[b][c] = mk(ge[3 * NVC + 3 * b + c], ge[ODIR + 3 * b + c]);
            qp_geometry<NVC, QUAD, false>(X, zero, stab.N1[q], stab.dN1[q], g);
            QPD s;
            qp_shape_dual<NVC, QUAD>(X, Uh, stab.dN1[q], g, s);
            const double wdet = stab.w[q] * g.det, wdetS = stab.wS[q] * g.det;
            const GenD sw = strains_dual<NPC, NVC>(stab, q, g, s, xe);
            const GenD t = stress_dual<LAMLAW>(sw, interp<NVC>(stab.N1[q], ge + 6 * NVC), interp<NVC>(stab.N1[q], ge + 7 * NVC),
                                               interp<NVC>(stab.N1[q], ge + 8 * NVC), slam[LAMLAW ? row : 0], hK, wdetS, wdet, s.Ju);
            strains_T_dual<NPC, NVC>(stab, q, g, s, t, ye);
            // - d/d eps int N_a f J dx
            const double wj = wdet * s.Ju.d;
            double fq[3] = {0, 0, 0};
#pragma unroll
            for (int b = 0; b < NVC; ++b)
#pragma unroll
                for (int c = 0; c < 3; ++c) fq[c] += stab.N1[q][b] * ge[OF + 3 * b + c];
#pragma unroll
            for (int a = 0; a < NPC; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) ye[3 * a + c] -= wj * stab.N2[q][a] * fq[c];
        } else {
            const double (*Uh)[3] = reinterpret_cast<const double (*)[3]>(ge + 3 * NVC);
            qp_geometry<NVC, QUAD, UHAT>(X, Uh, stab.N1[q], stab.dN1[q], g);
            if constexpr (MODE == JVP_LOAD) {
                const double wj = stab.w[q] * g.det * g.Ju;
                double fq[3] = {0, 0, 0};
#pragma unroll
                for (int b = 0; b < NVC; ++b)
#pragma unroll
                    for (int c = 0; c < 3; ++c) fq[c] += stab.N1[q][b] * ge[ODIR + 3 * b + c];
#pragma unroll
                for (int a = 0; a < NPC; ++a)
#pragma unroll
                    for (int c = 0; c < 3; ++c) ye[3 * a + c] -= wj * stab.N2[q][a] * fq[c];
            } else {
                Mat mat, ex;
                const Gen s = strains_q<NPC, NVC>(stab, q, g, xe);
                Gen t;
                if constexpr (MODE == JVP_LAM) {
                    lam_measures(hK, stab.wS[q] * g.det, stab.w[q] * g.det, g.Ju, mat);
                    t = stress_lam(s, mat, slam[row]);
                } else {
                    material<MODE>(interp<NVC>(stab.N1[q], ge + 6 * NVC), interp<NVC>(stab.N1[q], ge + 7 * NVC),
                                   interp<NVC>(stab.N1[q], ge + 8 * NVC), hK, stab.wS[q] * g.det, stab.w[q] * g.det, g.Ju, mat, ex);
                    const double dq = interp<NVC>(stab.N1[q], ge + ODIR);
                    mat.cm *= dq; mat.cb *= dq; mat.cs *= dq; mat.cd *= dq;
                    t = stress_of(s, mat);
                    if constexpr (MODE == JVP_NU) {
                        ex.cm *= dq; ex.cb *= dq;
                        stress_add_dnu(s, ex, t);
                    }
                }
                strains_T_q<NPC, NVC>(stab, q, g, t, ye);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < LD; ++i) ye[i] = quad_xor_sum(ye[i]);
    double* out = ybuf + (size_t)pos * YSTRIDE;
#pragma unroll
    for (int i = 0; i < LD; ++i)
        if ((i % 4) == sub) out[i] = ye[i];
}

// Forward counterpart of k_shape_gradient_penalty: out += d/d eps [P(uhat + eps dir)] x for the facets flist[0 .. nlist), x = w - g.
// P = beta/h_K int |J F^-T N| (.,.) ds depends on uhat through Nanson's factor only (the cell diameter belongs to the reference
// configuration).  One thread per facet, plain read-modify-write of out: the facets of ONE launch share no node (the host colours them),
// and the launches follow each other in the stream, so the order of the additions is fixed.
template <int NVC, bool QUAD, bool CG1>
__global__ void k_jvp_penalty(MeshDev m, FieldsDev f, FacetDev fd, double beta, const int* __restrict__ flist, int nlist,
                              const double* __restrict__ x, const double* __restrict__ dir, double* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nlist) return;
    const int i = flist[t];
    const int e = fd.cell[i], k = fd.ledge[i];
    double X[NVC][3];
    D1 Uh[NVC][3];
    for (int b = 0; b < NVC; ++b) {
        const int v = m.cells[b * m.nel + e];
        for (int c = 0; c < 3; ++c) {
            X[b][c] = m.xyz[3 * v + c];
            Uh[b][c] = mk(f.uhat[3 * v + c], dir[3 * v + c]);
        }
    }
    const int ka = k, kb = (k + 1) % NVC;
    double tv[3], len = 0.0;
    for (int c = 0; c < 3; ++c) {
        tv[c] = X[kb][c] - X[ka][c];
        len += tv[c] * tv[c];
    }
    len = sqrt(len);
    for (int c = 0; c < 3; ++c) tv[c] /= len;
    const int un[3] = {fd.unode[3 * i], fd.unode[3 * i + 1], fd.unode[3 * i + 2]};
    const int vn[2] = {fd.vnode[2 * i], fd.vnode[2 * i + 1]};
    const double gs[3] = {-0.7745966692414834, 0.0, 0.7745966692414834};
    const double gw[3] = {0.5555555555555556, 0.8888888888888888, 0.5555555555555556};
    double ru[3][3] = {}, rt[3][3] = {};                // [local node][component]
    for (int q = 0; q < 3; ++q) {
        const double s = gs[q];
        double xi, eta, M[NVC], dM[NVC][2], zero[NVC][3] = {};
        edge_ref_point(QUAD, k, s, xi, eta);
        p1_shape<NVC, QUAD>(xi, eta, M, dM);
        QPG g;
        qp_geometry<NVC, QUAD, false>(X, zero, M, dM, g);
        QPD sd;
        qp_shape_dual<NVC, QUAD>(X, Uh, dM, g, sd);
        double Nf[3];
        cross3(tv, g.E2, Nf);
        D1 v[3];
        for (int a = 0; a < 3; ++a) v[a] = sd.cof[a][0] * Nf[0] + sd.cof[a][1] * Nf[1] + sd.cof[a][2] * Nf[2];
        const D1 nanson = dsqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        const double wq = gw[q] * 0.5 * len * beta / m.hK[e] * nanson.d;
        const double L1[2] = {0.5 * (1.0 - s), 0.5 * (1.0 + s)};
        const double L2[3] = {CG1 ? L1[0] : 0.5 * s * (s - 1.0), CG1 ? 0.0 : 1.0 - s * s, CG1 ? L1[1] : 0.5 * s * (s + 1.0)};
        double R[3];
        R[k % 3] = 1.0; R[(k + 1) % 3] = s; R[(k + 2) % 3] = -s;
        for (int c = 0; c < 3; ++c) {
            double xu = 0, xt = 0;
            for (int a = 0; a < 3; ++a) xu += L2[a] * x[3 * un[a] + c];
            for (int a = 0; a < 3; ++a) ru[a][c] += wq * L2[a] * xu;
            if (fd.MR) {
                // CG2CR1: the rotation's trace on edge k through all three Crouzeix-Raviart functions of the cell (k_penalty_setup)
                for (int a = 0; a < 3; ++a) xt += R[a] * x[m.ndof_u + 3 * fd.rnode[3 * i + a] + c];
                for (int a = 0; a < 3; ++a) rt[a][c] += wq * R[a] * xt;
            } else {
                for (int a = 0; a < 2; ++a) xt += L1[a] * x[m.ndof_u + 3 * vn[a] + c];
                for (int a = 0; a < 2; ++a) rt[a][c] += wq * L1[a] * xt;
            }
        }
    }
    for (int c = 0; c < 3; ++c) {
        for (int a = 0; a < 3; ++a)
            if (!(CG1 && a == 1)) out[3 * un[a] + c] += ru[a][c];           // CG1CG1: no mid-edge node
        if (fd.MR) {
            for (int a = 0; a < 3; ++a) out[m.ndof_u + 3 * fd.rnode[3 * i + a] + c] += rt[a][c];
        } else {
            for (int a = 0; a < 2; ++a) out[m.ndof_u + 3 * vn[a] + c] += rt[a][c];
        }
    }
}

}  // namespace femo
