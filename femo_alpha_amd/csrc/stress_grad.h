// Derivatives of the DG1 stress fields of stress.h (k_stress_field: "stress", "stress_mid", "stress_bot"), gfx950, fp64.
//
// Per cell e the field solves  M_e c_e = b_e  with  M_e = sum_q w_q det_q N_i N_j  and  b_e,i = sum_q w_q det_q N_i vm_q.
// det_q is the plain dx of the projection and comes from the reference coordinates alone (qp_geometry), so M_e depends on no
// argument and only vm_q has to be differentiated.  For a cotangent cbar (nvc * nel, cell-major like femo_field_output):
//   bbar_e = M_e^-1 cbar_e  (M_e symmetric),   vmbar_q = w_q det_q sum_i bbar_e,i N_i(q),
// and vmbar_q is pushed through vm_q -- what k_pnorm does with its weight wj rho p / vm, here with the surface factor zf
// (xi2 = zf h: z = zf h, the thickness-gradient term -zf b (x) gradx(h); for zf = 0 the thickness derivative is exactly zero).
//
// Zero stress: vm = sqrt(...) is not differentiable where vm_q = 0 (w = 0, or a point without strain); such a point contributes
// zero -- a subgradient, the convention of k_pnorm and k_shape_gradient.  Every derivative is finite at w = 0.
//
// No float atomics anywhere: every cell (or (cell, row) / (cell, uhat component)) writes its own slot and a fixed-order gather adds
// the slots per node (k_gather_sum for the state, k_vertex_gather for nodal fields and uhat), so the products are bitwise repeatable.
#pragma once
#include "shell_device.h"
#include "shape_sens.h"
#include "stress.h"

namespace femo {

// x <- M_e^-1 x,  M_e = sum_q w_q det_q N_i N_j of the reference geometry (the matrix of k_stress_field, eliminated the same way)
template <int NVC>
__device__ __forceinline__ void cell_mass_solve(const Tables& t, const double (*X)[3], double* x) {
    double A[NVC][NVC + 1];
    for (int i = 0; i < NVC; ++i) {
        for (int j = 0; j < NVC; ++j) A[i][j] = 0.0;
        A[i][NVC] = x[i];
    }
    for (int q = 0; q < t.nq; ++q) {
        double J0[3] = {0, 0, 0}, J1[3] = {0, 0, 0}, a[3];
        for (int b = 0; b < NVC; ++b)
            for (int c = 0; c < 3; ++c) {
                J0[c] += X[b][c] * t.dN1[q][b][0];
                J1[c] += X[b][c] * t.dN1[q][b][1];
            }
        cross3(J0, J1, a);
        const double wd = t.w[q] * sqrt(dot3(a, a));
        for (int i = 0; i < NVC; ++i)
            for (int j = 0; j < NVC; ++j) A[i][j] += wd * t.N1[q][i] * t.N1[q][j];
    }
    for (int k = 0; k < NVC; ++k) {
        const double ip = 1.0 / A[k][k];
        for (int i = k + 1; i < NVC; ++i) {
            const double fct = A[i][k] * ip;
            for (int j = k; j <= NVC; ++j) A[i][j] -= fct * A[k][j];
        }
    }
    for (int i = NVC - 1; i >= 0; --i) {
        double s = A[i][NVC];
        for (int j = i + 1; j < NVC; ++j) s -= A[i][j] * x[j];
        x[i] = s / A[i][i];
    }
}

// The cell's share of (d c_e / d arg)^T cbar_e for bbar = M_e^-1 cbar_e.
// mode 1: w (ye, LD entries in the element-vector order of k_pnorm);  2: h, 3: E, 4: nu (ge, NVC entries; entry 0 for per-cell fields)
template <int NPC, int NVC, bool QUAD, bool UHAT>
__device__ __forceinline__ void field_vjp_cell(const Tables& t, const Elem<NPC, NVC>& el, bool ewm, const double* xe, double zf, int mode,
                                               const double* bbar, double* ye, double* ge) {
    for (int q = 0; q < t.nq; ++q) {
        QPG g;
        qp_geometry<NVC, QUAD, UHAT>(el.X, el.Uh, t.N1[q], t.dN1[q], g);
        double vb = 0.0;
        for (int i = 0; i < NVC; ++i) vb += bbar[i] * t.N1[q][i];
        vb *= t.w[q] * g.det;                                       // vmbar_q
        const double hq = interp<NVC>(t.N1[q], el.hn), Eq = interp<NVC>(t.N1[q], el.En), nuq = interp<NVC>(t.N1[q], el.nun);
        const TopStrain ts = top_strain<NPC, NVC>(t, q, g, el.hn, ewm, xe, hq, zf);
        double sig[3];
        const double vm = von_mises(ts, Eq, nuq, sig);
        if (!(vm > 0.0)) continue;                                  // zero stress: zero contribution (subgradient)
        if (mode == 1) {
            double de[3];
            dvm_deps(sig, vm, Eq, nuq, de);
            Gen tt;
            const double z = zf * hq;
            tt.e00 = vb * de[0]; tt.e11 = vb * de[1]; tt.g01 = vb * de[2];
            tt.k00 = -z * tt.e00; tt.k11 = -z * tt.e11; tt.k01 = -z * tt.g01;
            tt.ga0 = tt.ga1 = tt.om = 0.0;
            strains_T_q<NPC, NVC>(t, q, g, tt, ye);
            // -zf b (x) gradx(h): b0 = -theta.E1, b1 = theta.E0, theta = sum_b NR_b theta_b (zero for per-cell thickness: gradx(h) = 0)
            const double cb0 = -zf * (tt.e00 * ts.gh0 + tt.g01 * ts.gh1), cb1 = -zf * (tt.e11 * ts.gh1 + tt.g01 * ts.gh0);
            for (int b = 0; b < NVC; ++b)
                for (int c = 0; c < 3; ++c) ye[3 * NPC + 3 * b + c] += t.NR[q][b] * (-cb0 * g.E1[c] + cb1 * g.E0[c]);
        } else if (mode == 2) {
            double de[3];
            dvm_deps(sig, vm, Eq, nuq, de);
            for (int b = 0; b < NVC; ++b) {
                const double Mb = ewm ? 1.0 : t.N1[q][b];
                double d0 = -zf * Mb * ts.k00, d1 = -zf * Mb * ts.k11, d2 = -zf * Mb * ts.k01;
                if (!ewm) {
                    const double r0 = t.dN1[q][b][0], r1 = t.dN1[q][b][1];
                    const double m0 = r0 * g.Q[0][0] + r1 * g.Q[1][0], m1 = r0 * g.Q[0][1] + r1 * g.Q[1][1];
                    d0 -= zf * ts.b0 * m0;
                    d1 -= zf * ts.b1 * m1;
                    d2 -= zf * (ts.b0 * m1 + ts.b1 * m0);
                }
                ge[b] += vb * (de[0] * d0 + de[1] * d1 + de[2] * d2);
                if (ewm) break;
            }
        } else if (mode == 3) {
            for (int b = 0; b < NVC; ++b) {
                ge[b] += vb * vm / Eq * (ewm ? 1.0 : t.N1[q][b]);
                if (ewm) break;
            }
        } else {
            const double om = 1.0 - nuq * nuq, c = Eq / om, dc = 2.0 * nuq * Eq / (om * om);
            const double ds0 = dc * (ts.e0 + nuq * ts.e1) + c * ts.e1, ds1 = dc * (nuq * ts.e0 + ts.e1) + c * ts.e0;
            const double ds2 = dc * 0.5 * (1.0 - nuq) * ts.g - 0.5 * c * ts.g;
            const double dv = ((2.0 * sig[0] - sig[1]) * ds0 + (2.0 * sig[1] - sig[0]) * ds1 + 6.0 * sig[2] * ds2) / (2.0 * vm);
            for (int b = 0; b < NVC; ++b) {
                ge[b] += vb * dv * (ewm ? 1.0 : t.N1[q][b]);
                if (ewm) break;
            }
        }
    }
}

template <int NPC, int NVC>
__device__ __forceinline__ void load_state(const MeshDev& m, const Elem<NPC, NVC>& el, const double* w, double* xe) {
    for (int a = 0; a < NPC; ++a)
        for (int c = 0; c < 3; ++c) xe[3 * a + c] = w[3 * el.pid[a] + c];
    for (int b = 0; b < NVC; ++b)
        for (int c = 0; c < 3; ++c) xe[3 * NPC + 3 * b + c] = w[m.ndof_u + 3 * rot_node(m, el, b) + c];
}

// Reverse product with respect to w (mode 1), h, E or nu (modes 2-4), one thread per cell.
// mode 1: the cell's LD results go to slot pos of ybuf (YSTRIDE doubles, the Morton order of eorder) for k_gather_sum.
// modes 2-4: per-cell fields are written to out[e] (one cell per entry); nodal fields leave NVC values per cell at
// cellbuf[NVC e + b] for k_vertex_gather.
template <int NPC, int NVC, bool QUAD, bool UHAT>
__global__ void __launch_bounds__(128)
k_field_vjp(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const int* __restrict__ eorder, const double* __restrict__ w, double zf,
            int mode, const double* __restrict__ cbar, double* __restrict__ ybuf, double* __restrict__ out) {
    constexpr int LD = 3 * NPC + 3 * NVC;
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= m.nel) return;
    const int e = eorder[pos];
    Elem<NPC, NVC> el;
    load_elem<NPC, NVC, UHAT>(m, f, e, el);
    double xe[LD], ye[LD], ge[NVC], bbar[NVC];
    load_state<NPC, NVC>(m, el, w, xe);
    for (int i = 0; i < NVC; ++i) bbar[i] = cbar[(size_t)NVC * e + i];
    cell_mass_solve<NVC>(*tab, el.X, bbar);
    for (int i = 0; i < LD; ++i) ye[i] = 0.0;
    for (int b = 0; b < NVC; ++b) ge[b] = 0.0;
    field_vjp_cell<NPC, NVC, QUAD, UHAT>(*tab, el, f.ewm != 0, xe, zf, mode, bbar, ye, ge);
    if (mode == 1) {
        double* dst = ybuf + (size_t)pos * YSTRIDE;
        for (int i = 0; i < LD; ++i) dst[i] = ye[i];
    } else if (f.ewm) {
        out[e] = ge[0];
    } else {
        for (int b = 0; b < NVC; ++b) ybuf[(size_t)NVC * e + b] = ge[b];
    }
}

// Partial Jacobian with respect to w (mode 1), h, E or nu (modes 2-4): one thread per row (e, i) = NVC e + i, which pushes the unit
// cotangent e_i through field_vjp_cell and writes its row -- W = LD entries (mode 1), NVC (nodal fields) or 1 (per-cell fields) at
// vals[W row], with the global columns in the element's local order.  Rows do not overlap: plain stores.
template <int NPC, int NVC, bool QUAD, bool UHAT>
__global__ void __launch_bounds__(128)
k_field_jac(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const double* __restrict__ w, double zf, int mode,
            double* __restrict__ vals, int* __restrict__ colidx) {
    constexpr int LD = 3 * NPC + 3 * NVC;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = gid / NVC, i = gid - e * NVC;
    if (e >= m.nel) return;
    Elem<NPC, NVC> el;
    load_elem<NPC, NVC, UHAT>(m, f, e, el);
    double xe[LD], ye[LD], ge[NVC], bbar[NVC];
    load_state<NPC, NVC>(m, el, w, xe);
    for (int k = 0; k < NVC; ++k) bbar[k] = k == i ? 1.0 : 0.0;
    cell_mass_solve<NVC>(*tab, el.X, bbar);
    for (int k = 0; k < LD; ++k) ye[k] = 0.0;
    for (int b = 0; b < NVC; ++b) ge[b] = 0.0;
    field_vjp_cell<NPC, NVC, QUAD, UHAT>(*tab, el, f.ewm != 0, xe, zf, mode, bbar, ye, ge);
    const size_t r = (size_t)gid;
    if (mode == 1) {
        double* v = vals + r * LD;
        int* ci = colidx + r * LD;
        for (int a = 0; a < NPC; ++a)
            for (int c = 0; c < 3; ++c) { v[3 * a + c] = ye[3 * a + c]; ci[3 * a + c] = 3 * el.pid[a] + c; }
        for (int b = 0; b < NVC; ++b)
            for (int c = 0; c < 3; ++c) {
                v[3 * NPC + 3 * b + c] = ye[3 * NPC + 3 * b + c];
                ci[3 * NPC + 3 * b + c] = m.ndof_u + 3 * rot_node(m, el, b) + c;
            }
    } else if (f.ewm) {
        vals[r] = ge[0];
        colidx[r] = e;
    } else {
        for (int b = 0; b < NVC; ++b) { vals[r * NVC + b] = ge[b]; colidx[r * NVC + b] = el.vid[b]; }
    }
}

// With respect to uhat, in forward-mode dual arithmetic like k_shape_gradient: one thread per (cell, uhat component dir = 3 b + c)
// forms  db_j = sum_q w_q det_q N_j d vm_q / d uhat_(b,c)  (det_q does not depend on uhat).
// cbar != null: reverse product, cellbuf[3 NVC e + dir] = (M_e^-1 cbar_e) . db  -> k_vertex_gather with three components;
// cbar == null: Jacobian column, M_e^-1 db into the rows NVC e + i at entry dir (row width 3 NVC), column 3 vertex + c.
template <int NPC, int NVC, bool QUAD>
__global__ void __launch_bounds__(128)
k_field_uhat(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const double* __restrict__ w, double zf, const double* __restrict__ cbar,
             double* __restrict__ cellbuf, double* __restrict__ vals, int* __restrict__ colidx) {
    constexpr int LD = 3 * NPC + 3 * NVC;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = gid / (3 * NVC), dir = gid - e * (3 * NVC);
    if (e >= m.nel) return;
    const int bseed = dir / 3, iseed = dir - 3 * bseed;
    Elem<NPC, NVC> el;
    load_elem<NPC, NVC, true>(m, f, e, el);
    D1 Uh[NVC][3];
    for (int b = 0; b < NVC; ++b)
        for (int i = 0; i < 3; ++i) Uh[b][i] = mk(el.Uh[b][i], (b == bseed && i == iseed) ? 1.0 : 0.0);
    double we[LD], db[NVC];
    load_state<NPC, NVC>(m, el, w, we);
    for (int j = 0; j < NVC; ++j) db[j] = 0.0;
    const int nq = tab->nq;
    for (int q = 0; q < nq; ++q) {
        QPG g;
        double zero[NVC][3] = {};
        qp_geometry<NVC, QUAD, false>(el.X, zero, tab->N1[q], tab->dN1[q], g);
        QPD s;
        qp_shape_dual<NVC, QUAD>(el.X, Uh, tab->dN1[q], g, s);
        const double hq = interp<NVC>(tab->N1[q], el.hn), Eq = interp<NVC>(tab->N1[q], el.En), nuq = interp<NVC>(tab->N1[q], el.nun);
        const GenD sw = strains_dual<NPC, NVC>(*tab, q, g, s, we);
        double th[3] = {0, 0, 0};
        D1 gh0 = mk(0.0), gh1 = mk(0.0);
        for (int b = 0; b < NVC; ++b) {
            for (int c = 0; c < 3; ++c) th[c] += tab->NR[q][b] * we[3 * NPC + 3 * b + c];
            if (!f.ewm) {
                const double r0 = tab->dN1[q][b][0], r1 = tab->dN1[q][b][1];
                gh0 = gh0 + el.hn[b] * (r0 * s.Q[0][0] + r1 * s.Q[1][0]);
                gh1 = gh1 + el.hn[b] * (r0 * s.Q[0][1] + r1 * s.Q[1][1]);
            }
        }
        const double b0 = -dot3(th, g.E1), b1 = dot3(th, g.E0), z = zf * hq;
        const D1 e0 = sw.e00 - z * sw.k00 - (zf * b0) * gh0;
        const D1 e1 = sw.e11 - z * sw.k11 - (zf * b1) * gh1;
        const D1 gg = sw.g01 - z * sw.k01 - zf * (b0 * gh1 + b1 * gh0);
        const double cc = Eq / (1.0 - nuq * nuq);
        const D1 s0 = cc * (e0 + nuq * e1), s1 = cc * (nuq * e0 + e1), s2 = (cc * 0.5 * (1.0 - nuq)) * gg;
        const D1 vm = dsqrt(s0 * s0 - s0 * s1 + s1 * s1 + 3.0 * (s2 * s2));
        if (!(vm.v > 0.0)) continue;                                // zero stress: zero contribution (subgradient)
        const double wd = tab->w[q] * g.det;
        for (int j = 0; j < NVC; ++j) db[j] += wd * tab->N1[q][j] * vm.d;
    }
    if (cbar) {
        double bbar[NVC];
        for (int i = 0; i < NVC; ++i) bbar[i] = cbar[(size_t)NVC * e + i];
        cell_mass_solve<NVC>(*tab, el.X, bbar);
        double s = 0.0;
        for (int j = 0; j < NVC; ++j) s += bbar[j] * db[j];
        cellbuf[(size_t)3 * NVC * e + dir] = s;
    } else {
        cell_mass_solve<NVC>(*tab, el.X, db);
        for (int i = 0; i < NVC; ++i) {
            const size_t k = ((size_t)NVC * e + i) * (3 * NVC) + dir;
            vals[k] = db[i];
            colidx[k] = 3 * el.vid[bseed] + iseed;
        }
    }
}

// out[ncomp v + c] = sum over the cells around vertex v, in the fixed order of the incidence list (v2e_ent = e * NVC + local vertex),
// of cellbuf[ncomp ent + c]
__global__ void __launch_bounds__(256)
k_vertex_gather(int nn, int ncomp, const int* __restrict__ v2e_off, const int* __restrict__ v2e_ent, const double* __restrict__ cellbuf,
                double* __restrict__ out) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= nn * ncomp) return;
    const int v = gid / ncomp, c = gid - v * ncomp;
    double s = 0.0;
    for (int k = v2e_off[v]; k < v2e_off[v + 1]; ++k) s += cellbuf[(size_t)ncomp * v2e_ent[k] + c];
    out[gid] = s;
}

}  // namespace femo
