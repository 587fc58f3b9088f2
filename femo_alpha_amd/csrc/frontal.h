// Multifrontal Cholesky of the shell operator on gfx950 (fp64): numeric factorisation and the
// triangular solves used as the PCG preconditioner.
//
// Role in the reference: PETSc KSP 'preonly' + PC 'lu' with MUMPS
// (reference femo_alpha/fea/utils_dolfinx.py:466,495-531) -- itself a multifrontal method.
// Here the elimination tree comes from a geometric nested dissection of the elements
// (femo_alpha_amd/solver/symbolic.py); element matrices are summed straight into the leaf fronts;
// every level of the tree is factorised by batched, blocked partial Cholesky kernels whose grids span
// all fronts of the level: parents are gathered from their children's Schur complements, then per
// outer panel of 128 columns the diagonal block is factorised and inverted by one workgroup per front
// (32x32 register Cholesky + fp64 MFMA), the rows below become factor rows by one GEMM against that
// inverse, and 64x64 tiles receive the rank-k updates on the matrix cores (right-looking with
// look-ahead at the top of the tree, left-looking on the levels with many fronts).
//
// Storage: a front is a dense nf x nf matrix of which only the lower triangle is maintained, kept in two places.  Its
// first npiv columns -- [L11; L21] after factorisation, i.e. the factor itself -- live for good in the panel store P
// (column-major, leading dimension nf, at P + poff[t]).  The trailing nb x nb block, the Schur complement that only the
// parent's extend-add consumes, lives in an arena S (leading dimension nb, at S + soff[t]) whose regions are reused
// as the factorisation climbs the tree (one region per parent level, placed at plan time so that regions alive together
// never overlap): 5.4 GB instead of 14.9 GB of square fronts at 1 M DOF.  Kernels address both through FrontView.  Linv keeps the inverses of the NB x NB diagonal
// blocks of L11, Sinv those of the 128 x 128 diagonal blocks (levels with few fronts), so that every
// triangular solve becomes a GEMV.
#pragma once
#include "shell_device.h"

namespace femo {

constexpr int NB = 32;     // panel width
constexpr int TS = 64;     // trailing-update tile
constexpr int NBO = 128;   // outer panel: the wide trailing update applies this many factor columns per pass
constexpr int SPD = 128;   // leading dimension of the stored diagonal-block inverses (== SP of the solve kernels)

struct FrontDev {
    int ntree;
    const int* nf;
    const int* npiv;
    const long long* poff;      // doubles, [ntree+1]: pivot columns of front t in P (nf x npiv, leading dimension nf)
    const long long* soff;      // doubles, [ntree]: Schur complement of front t in S (nb x nb, leading dimension nb)
    const long long* doff;      // ints, [ntree+1]
    const int* dofs;            // global DOF of every front row
    const int* upmap;           // row of the parent front (boundary rows only)
    const int* parent;
    const int* child[2];        // left / right
    const int* cinv[2];         // per front row: the row of the left / right child's front that lands there, or -1
    const int* cmono;           // per front: bit 0 / 1 = the left / right child's rows land in increasing rows (child_maps.h); 0 = general gather
    const long long* linvoff;   // doubles, [ntree+1]
    const long long* xoff;      // doubles, [ntree+1]: where the front's X = L11^-1 starts (fronts of the wide levels)
    double* P;
    double* S;
    double* Linv;
    double* X;                  // L11^-1, lower triangle, column-major with leading dimension ldx_of(npiv)
    double* Xtmp;               // scratch of the same shape (the products C XA of the recursive inversion)
};

// entries of one front by FRONT row and column (r >= c): pivot columns in the panel store, the rest in the Schur arena
// leading dimension of the pivot columns in the panel store: nf rounded up to even, so that every column starts on a
// 16-byte boundary and the rank-k update can stage two rows of a factor column per load (the pad row stays zero)
__device__ __host__ inline int ldp_of(int nf) { return (nf + 1) & ~1; }

struct FrontView {
    double* P;
    double* S;
    int nf, np;
    __device__ __forceinline__ double* col(int c) const {
        return c < np ? P + (size_t)ldp_of(nf) * c : S + (size_t)(nf - np) * (c - np) - np;     // then [r], r >= c
    }
};
__device__ __forceinline__ FrontView front_view(const FrontDev& fd, int t) {
    FrontView v;
    v.nf = fd.nf[t]; v.np = fd.npiv[t];
    v.P = fd.P + fd.poff[t];
    v.S = fd.S + fd.soff[t];
    return v;
}

// leading dimension of a front's X (a multiple of the 128-column outer panel, so that k_diag_block can write the
// inverse of every diagonal block straight into place)
__device__ __host__ inline int ldx_of(int np) { return (np + SPD - 1) / SPD * SPD; }

// ------------------------------------------------------------------------------------------ assembly
// one wave per element; lane j evaluates column j of K_e (operator applied to e_j) and adds its
// lower-triangle entries into the element's leaf front.  Masked (strong-BC) rows/columns are skipped.
template <int NPC, int NVC, bool QUAD, bool UHAT, bool MASS, bool LAM = false>
__global__ void __launch_bounds__(64)          // 239 registers, two waves per SIMD; capped at 167 (three waves, 52 B of scratch): 1.33 against 1.07 ms
k_front_assemble(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, double aK, double aM, FrontDev fd,
                 const int* __restrict__ elem_front, const int* __restrict__ elem_map, const unsigned char* __restrict__ mask,
                 const double* __restrict__ eq) {
    constexpr int LD = 3 * NPC + 3 * NVC;
    const int e = blockIdx.x;
    const int j = threadIdx.x;
    if (e >= m.nel) return;
    Elem<NPC, NVC> el;
    load_elem<NPC, NVC, UHAT>(m, f, e, el);
    // the quadrature-point data all lanes share: computed once, by lane q for point q, and parked in LDS (stage_qpoints)
    extern __shared__ double sq_raw[];
    QPoint<NPC, NVC>* sq = reinterpret_cast<QPoint<NPC, NVC>*>(sq_raw);
    stage_qpoints<NPC, NVC, QUAD, UHAT, LAM>(tab, el, aK, j, 64, sq);
    if (j >= LD) return;
    const double* L = LAM ? f.clt + (size_t)LAM_W * e : nullptr;     // laminate mode: the cell's values, uniform over the wave
    double ye[LD];
#pragma unroll
    for (int i = 0; i < LD; ++i) ye[i] = 0.0;
    // the lane's unit vector e_j: displacement component cj of P2 node aj, or rotation component cj of vertex aj
    const bool is_u = j < 3 * NPC;
    const int aj = is_u ? j / 3 : (j - 3 * NPC) / 3;
    const int cj = j - 3 * (is_u ? aj : NPC + aj);
    const int nq = tab->nq;
    for (int q = 0; q < nq; ++q) {
        const QPoint<NPC, NVC>& p = sq[q];
        // strains of e_j without the 39-entry reduction: the reduced vectors are scalar multiples of one unit vector;
        // the lane reads its own node's table row (a per-lane index into d[][] would send the array to scratch)
        const double r0 = is_u ? tab->dN2[q][aj][0] : tab->dNR[q][aj][0], r1 = is_u ? tab->dN2[q][aj][1] : tab->dNR[q][aj][1];
        const double dk0 = r0 * p.g.Q[0][0] + r1 * p.g.Q[1][0], dk1 = r0 * p.g.Q[0][1] + r1 * p.g.Q[1][1];
        const double Mj = is_u ? 0.0 : tab->NR[q][aj];
        double G0[3], G1[3], th[3], T0[3], T1[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double ec = (c == cj) ? 1.0 : 0.0;
            G0[c] = is_u ? dk0 * ec : 0.0;
            G1[c] = is_u ? dk1 * ec : 0.0;
            th[c] = Mj * ec;
            T0[c] = is_u ? 0.0 : dk0 * ec;
            T1[c] = is_u ? 0.0 : dk1 * ec;
        }
        const Gen s = strains_reduced(p.g, G0, G1, th, T0, T1);
        const Gen t = law<LAM>(s, p.mat, L);
        strains_T<NPC, NVC>(p.g, p.d, p.mm, tab->NR[q], t, ye);
    }
    if (MASS) {
        // The inertia term in a loop of its own (compiled out of the static operator): inside the stiffness loop its live values pushed
        // the kernel from 239 registers past 256 and to ONE wave per SIMD (front assembly of config 5: 1.95 against 1.09 ms).  Column j
        // of the element mass matrix, written out for the unit vector e_j: entries only where the component matches, N_i N_j for the
        // displacement, h_K^2 N_i N_j for the rotation (mass_qp)
        double rhon[NVC];
#pragma unroll
        for (int b = 0; b < NVC; ++b) rhon[b] = f.rho[f.ewm ? e : el.vid[b]];
        const double hk2 = is_u ? 1.0 : el.hK * el.hK;
        for (int q = 0; q < nq; ++q) {
            const QPoint<NPC, NVC>& p = sq[q];
            double rq = 0.0;
#pragma unroll
            for (int b = 0; b < NVC; ++b) rq += tab->N1[q][b] * rhon[b];
            const double cmj = aM * rq * p.hq * tab->w[q] * p.g.det * p.g.Ju * hk2 * (is_u ? tab->N2[q][aj] : tab->NR[q][aj]);
#pragma unroll
            for (int a = 0; a < NPC; ++a)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) ye[3 * a + cc] += (is_u && cc == cj) ? cmj * tab->N2[q][a] : 0.0;
#pragma unroll
            for (int b = 0; b < NVC; ++b)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) ye[3 * NPC + 3 * b + cc] += (!is_u && cc == cj) ? cmj * tab->NR[q][b] : 0.0;
        }
    }
    const int t = elem_front[e];
    const FrontView fv = front_view(fd, t);
    const int* map = elem_map + (size_t)e * LD;
    const int* gd = fd.dofs + fd.doff[t];
    // K_e is symmetric: the lane's column j is also row j.  Adding it as a ROW makes the 39 lanes of one atomic
    // instruction hit one column of the front (a few cache lines) instead of 39 different columns.
    const int pj = map[j];
    if (mask && mask[gd[pj]]) return;
    // eq (option "equilibrate", an experiment): the matrix factorised is D K D with D = diag(eq)
    const double sj = eq ? eq[gd[pj]] : 1.0;
#pragma unroll
    for (int i = 0; i < LD; ++i) {
        const int pi = map[i];
        if (pj >= pi && !(mask && mask[gd[pi]])) atomicAdd(fv.col(pi) + pj, eq ? ye[i] * sj * eq[gd[pi]] : ye[i]);
    }
}

// ---- front-centric assembly (r5, option "assemble_fc"): ONE workgroup per leaf front.
// k_front_assemble is bound by the memory side: float atomics never execute in L2 on this chip (MI355X_MICROARCH.md, "Global float
// atomics": every wave-instruction leaves L2 as one uncached 64-byte request per segment it touches, ~20 G requests/s chip-wide), and a
// column of K_e lands on ~10 segments of its front -- 26 M requests, 1.3 of the kernel's 1.43 ms at 1 M DOF, whatever the arithmetic
// does (threads sharing the quadrature points of a column changed nothing).  Here a front belongs to one workgroup for the whole
// kernel: it zeroes the front (no k_zero_fronts launch), then takes the front's elements ONE AFTER THE OTHER -- thread (j, part)
// evaluates column j of K_e over every PARTS-th quadrature point (39 x 3 of 128 threads on quadrilaterals, 27 x 2 of 64 on triangles:
// one wave per element used 39 / 27 of its 64 lanes), the partial columns meet in LDS, and the sums are added to the front with
// plain loads and stores: no other workgroup touches this front, and the elements of one front are separated by workgroup barriers.
// The front is written in L2 and leaves it once.
__device__ __host__ constexpr int assemble_block(int ld) { return ld > 32 ? 128 : 64; }
__device__ __host__ constexpr size_t assemble_lds(int ld, size_t qpoint_bytes) {   // the staged points, then the partial columns in the same place
    const size_t part = (size_t)(assemble_block(ld) / ld) * ld * (ld | 1) * sizeof(double);
    return part > qpoint_bytes ? part : qpoint_bytes;
}
template <int NPC, int NVC, bool QUAD, bool UHAT, bool MASS, bool LAM = false>
__global__ void __launch_bounds__(assemble_block(3 * NPC + 3 * NVC))
k_front_assemble_fc(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, double aK, double aM, FrontDev fd,
                    const int* __restrict__ level_nodes, const int* __restrict__ fel_off, const int* __restrict__ fel,
                    const int* __restrict__ elem_map, const unsigned char* __restrict__ mask, const double* __restrict__ eq) {
    constexpr int LD = 3 * NPC + 3 * NVC;
    constexpr int BLK = assemble_block(LD), PARTS = BLK / LD, PS = LD | 1, NK = (LD + PARTS - 1) / PARTS;
    const int slot = blockIdx.x;
    const int t = level_nodes[slot];
    const int tid = threadIdx.x;
    const int part = tid / LD, j = tid - part * LD;           // part == PARTS: the lanes left over (they zero and stage, nothing else)
    const bool work = part < PARTS;
    const FrontView fv = front_view(fd, t);
    const int nf = fv.nf, np = fv.np;
    // the front starts from zero: its pivot columns (rows c.. of column c; the pad row of an odd front stays as it is) and its Schur block
    {
        const int ldp = ldp_of(nf);
        for (int c = 0; c < np; ++c) {
            double* col = fv.P + (size_t)ldp * c;
            for (int r = c + tid; r < nf; r += BLK) col[r] = 0.0;
        }
        const int nb = nf - np;
        for (int c = 0; c < nb; ++c) {
            double* col = fv.S + (size_t)nb * c;
            for (int r = c + tid; r < nb; r += BLK) col[r] = 0.0;
        }
    }
    extern __shared__ double sq_raw[];
    QPoint<NPC, NVC>* sq = reinterpret_cast<QPoint<NPC, NVC>*>(sq_raw);
    double* pb = sq_raw;                                      // partial columns: [part][j][i], rows of PS doubles (odd: conflict-free)
    const int* gd = fd.dofs + fd.doff[t];
    const bool is_u = j < 3 * NPC;
    const int aj = is_u ? j / 3 : (j - 3 * NPC) / 3;
    const int cj = j - 3 * (is_u ? aj : NPC + aj);
    const int e0 = fel_off[slot], e1 = fel_off[slot + 1];
    for (int ei = e0; ei < e1; ++ei) {
        const int e = fel[ei];
        Elem<NPC, NVC> el;
        load_elem<NPC, NVC, UHAT>(m, f, e, el);
        __syncthreads();                                      // the previous element's partial columns have been read (and the zero fill is done)
        stage_qpoints<NPC, NVC, QUAD, UHAT, LAM>(tab, el, aK, tid, BLK, sq);
        const double* L = LAM ? f.clt + (size_t)LAM_W * e : nullptr;
        double ye[LD];
#pragma unroll
        for (int i = 0; i < LD; ++i) ye[i] = 0.0;
        const int nq = work ? tab->nq : 0;
        for (int q = part; q < nq; q += PARTS) {
            const QPoint<NPC, NVC>& p = sq[q];
            const double r0 = is_u ? tab->dN2[q][aj][0] : tab->dNR[q][aj][0], r1 = is_u ? tab->dN2[q][aj][1] : tab->dNR[q][aj][1];
            const double dk0 = r0 * p.g.Q[0][0] + r1 * p.g.Q[1][0], dk1 = r0 * p.g.Q[0][1] + r1 * p.g.Q[1][1];
            const double Mj = is_u ? 0.0 : tab->NR[q][aj];
            double G0[3], G1[3], th[3], T0[3], T1[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double ec = (c == cj) ? 1.0 : 0.0;
                G0[c] = is_u ? dk0 * ec : 0.0;
                G1[c] = is_u ? dk1 * ec : 0.0;
                th[c] = Mj * ec;
                T0[c] = is_u ? 0.0 : dk0 * ec;
                T1[c] = is_u ? 0.0 : dk1 * ec;
            }
            const Gen s = strains_reduced(p.g, G0, G1, th, T0, T1);
            // the laminate is re-read per point (scalar loads): hoisted out of the loop its 21 values cost the kernel its second wave per SIMD
            const double* Lq = L;
            if constexpr (LAM) asm volatile("" : "+s"(Lq));
            const Gen tt = law<LAM>(s, p.mat, Lq);
            strains_T<NPC, NVC>(p.g, p.d, p.mm, tab->NR[q], tt, ye);
        }
        if (MASS) {
            double rhon[NVC];
#pragma unroll
            for (int b = 0; b < NVC; ++b) rhon[b] = f.rho[f.ewm ? e : el.vid[b]];
            const double hk2 = is_u ? 1.0 : el.hK * el.hK;
            for (int q = part; q < nq; q += PARTS) {
                const QPoint<NPC, NVC>& p = sq[q];
                double rq = 0.0;
#pragma unroll
                for (int b = 0; b < NVC; ++b) rq += tab->N1[q][b] * rhon[b];
                const double cmj = aM * rq * p.hq * tab->w[q] * p.g.det * p.g.Ju * hk2 * (is_u ? tab->N2[q][aj] : tab->NR[q][aj]);
#pragma unroll
                for (int a = 0; a < NPC; ++a)
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) ye[3 * a + cc] += (is_u && cc == cj) ? cmj * tab->N2[q][a] : 0.0;
#pragma unroll
                for (int b = 0; b < NVC; ++b)
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) ye[3 * NPC + 3 * b + cc] += (!is_u && cc == cj) ? cmj * tab->NR[q][b] : 0.0;
            }
        }
        __syncthreads();                                      // every thread is through with the staged points
        if (work) {
#pragma unroll
            for (int i = 0; i < LD; ++i) pb[((size_t)part * LD + j) * PS + i] = ye[i];
        }
        __syncthreads();
        if (work) {
            // thread (j, part) adds the rows i = part, part + PARTS, ... of column j (K_e is symmetric: as ROW j of the front's column i,
            // so that the threads of a wave write along a column)
            const int* map = elem_map + (size_t)e * LD;
            const int pj = map[j];
            const bool mj = mask && mask[gd[pj]];
            const double sj = eq ? eq[gd[pj]] : 1.0;
            double* dst[NK];
            bool ok[NK];
            double v[NK], old[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int i = min(part + PARTS * k, LD - 1);
                const int pi = map[i];
                ok[k] = part + PARTS * k < LD && pj >= pi && !mj && !(mask && mask[gd[pi]]);
                double x = 0.0;
#pragma unroll
                for (int pp = 0; pp < PARTS; ++pp) x += pb[((size_t)pp * LD + j) * PS + i];
                v[k] = eq ? x * sj * eq[gd[pi]] : x;
                dst[k] = ok[k] ? fv.col(pi) + pj : fd.P;         // (unconditional loads from a safe address: all of them in flight at once)
            }
#pragma unroll
            for (int k = 0; k < NK; ++k) old[k] = *dst[k];
#pragma unroll
            for (int k = 0; k < NK; ++k) if (ok[k]) *dst[k] = old[k] + v[k];
        }
    }
}

// penalty facet blocks into the leaf front of the facet's element
__global__ void k_front_penalty(FacetDev pf, FrontDev fd, const int* __restrict__ elem_front, const int* __restrict__ elem_map,
                                int ld, int npc, int nvc, const unsigned char* __restrict__ mask, const double* __restrict__ eq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pf.nf) return;
    const int e = pf.cell[i], k = pf.ledge[i];
    const int t = elem_front[e];
    const FrontView fv = front_view(fd, t);
    const int* map = elem_map + (size_t)e * ld;
    const int* gd = fd.dofs + fd.doff[t];
    const int kb = (k + 1) % nvc;
    const int un[3] = {k, npc == nvc ? k : nvc + k, kb};          // element-local P2 nodes (a, mid, b); CG1CG1: no mid node, its slot of M2 is empty
    const int vn[2] = {k, kb};                   // element-local vertices
    for (int c = 0; c < 3; ++c) {
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                const int pa = map[3 * un[a] + c], pb = map[3 * un[b] + c];
                if (pa >= pb && !(mask && (mask[gd[pa]] || mask[gd[pb]])))
                    atomicAdd(fv.col(pb) + pa, pf.M2[9 * i + 3 * a + b] * (eq ? eq[gd[pa]] * eq[gd[pb]] : 1.0));
            }
        if (pf.MR) {
            // CG2CR1: the 3 x 3 rotation block over the cell's three edge midpoints (element-local rotation slots 0, 1, 2)
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    const int pa = map[3 * npc + 3 * a + c], pb = map[3 * npc + 3 * b + c];
                    if (pa >= pb && !(mask && (mask[gd[pa]] || mask[gd[pb]])))
                        atomicAdd(fv.col(pb) + pa, pf.MR[9 * i + 3 * a + b] * (eq ? eq[gd[pa]] * eq[gd[pb]] : 1.0));
                }
        } else
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) {
                const int pa = map[3 * npc + 3 * vn[a] + c], pb = map[3 * npc + 3 * vn[b] + c];
                if (pa >= pb && !(mask && (mask[gd[pa]] || mask[gd[pb]])))
                    atomicAdd(fv.col(pb) + pa, pf.M1[4 * i + 2 * a + b] * (eq ? eq[gd[pa]] * eq[gd[pb]] : 1.0));
            }
    }
}

// unit diagonal for masked pivots (their rows / columns were skipped during assembly)
__global__ void k_front_mask_diag(FrontDev fd, const unsigned char* __restrict__ mask) {
    const int t = blockIdx.x;
    const int np = fd.npiv[t], nf = fd.nf[t];
    double* P = fd.P + fd.poff[t];
    const int* gd = fd.dofs + fd.doff[t];
    for (int p = threadIdx.x; p < np; p += blockDim.x)
        if (mask[gd[p]]) P[p + (size_t)ldp_of(nf) * p] = 1.0;
}

// lower triangle of every front of a level := 0 (the leaf fronts before the element matrices are added)
__global__ void __launch_bounds__(256)
k_zero_fronts(FrontDev fd, const int* __restrict__ level_nodes, int first) {
    const int t = level_nodes[first + blockIdx.y];
    const int nf = fd.nf[t];
    const int nt = (nf + TS - 1) / TS;
    const int lin = blockIdx.x;
    if (lin >= nt * (nt + 1) / 2) return;
    int ti = (int)((sqrt(8.0 * lin + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= lin) ++ti;
    while (ti * (ti + 1) / 2 > lin) --ti;
    const int tj = lin - ti * (ti + 1) / 2;
    const FrontView fv = front_view(fd, t);
    const int r0 = ti * TS, c0 = tj * TS;
    for (int idx = threadIdx.x; idx < TS * TS; idx += blockDim.x) {
        const int r = r0 + idx % TS, cc = c0 + idx / TS;
        if (r < nf && cc <= r) fv.col(cc)[r] = 0.0;
    }
}

// extend-add as a gather: every entry of the parent's lower triangle is the sum of the entries of its children's
// Schur complements that land there (row maps cinv) -- written once, never read: no zero fill of the parent, no
// read-modify-write, one launch per level for both children.  Masked (strong-BC) pivots get their unit diagonal here.
__global__ void __launch_bounds__(256)
k_extend_gather(FrontDev fd, const int* __restrict__ level_nodes, int first, const unsigned char* __restrict__ mask, int skip_schur) {
    const int p = level_nodes[first + blockIdx.y];
    const int ch0 = fd.child[0][p], ch1 = fd.child[1][p];
    if (ch0 < 0 && ch1 < 0) return;                      // nothing below: the front keeps what it was given
    const int nfp = fd.nf[p], npp = fd.npiv[p];
    const int nt = (nfp + TS - 1) / TS;
    const int lin = blockIdx.x;
    if (lin >= nt * (nt + 1) / 2) return;
    int ti = (int)((sqrt(8.0 * lin + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= lin) ++ti;
    while (ti * (ti + 1) / 2 > lin) --ti;
    const int tj = lin - ti * (ti + 1) / 2;
    const int r0 = ti * TS, c0 = tj * TS;
    // skip_schur: only the first outer panel's columns are filled here -- every other column of this level's fronts is
    // gathered from the children by the rank-k update that touches it first (k_trailing_mfma<true>); fronts without
    // pivots have no such update
    const int c_end = (skip_schur && npp > 0) ? min(npp, NBO) : nfp;
    if (c0 >= c_end) return;
    __shared__ int rmap[2][TS], cmap[2][TS];
    const long long dp = fd.doff[p];
    for (int i = threadIdx.x; i < 4 * TS; i += blockDim.x) {
        const int side = (i / TS) & 1, isc = i / (2 * TS), k = i % TS;
        const int g = (isc ? c0 : r0) + k;
        const int v = (g < nfp && (side ? ch1 : ch0) >= 0) ? fd.cinv[side][dp + g] : -1;
        if (isc) cmap[side][k] = v; else rmap[side][k] = v;
    }
    __syncthreads();
    const FrontView fp = front_view(fd, p);
    // the children are read in their Schur complements only (rows and columns beyond their pivots)
    const FrontView f0 = front_view(fd, ch0 >= 0 ? ch0 : p), f1 = front_view(fd, ch1 >= 0 ? ch1 : p);
    const int* gd = fd.dofs + dp;
    // a thread owns row lr of the tile and 16 of its columns: all child reads are issued before the first store
    const int lr = threadIdx.x % TS, lc0 = threadIdx.x / TS;
    const int r = r0 + lr;
    const int ra0 = rmap[0][lr], ra1 = rmap[1][lr];
    double v[TS / 4];
    if (fd.cmono[p] == 3) {
        // Both children land in increasing rows (child_maps.h): for cc <= r the child rows are ordered as they stand, the entry is
        // S_c[(row's - np_c) + nb_c (column's - np_c)].  A wave holds ONE column per k (lc0 is the wave's number), so the column term
        // is scalar arithmetic on the child's base pointer and a thread adds one row offset, the same for all its 16 entries.
        // Absent rows and columns are clamped to the first entry of the child's block and the value is zeroed afterwards: no select
        // on an address, all loads in flight before the first use.  cc <= r needs testing only in the tiles on the diagonal.
        const bool diag = ti == tj;
        double g[2][TS / 4];
#pragma unroll
        for (int sd = 0; sd < 2; ++sd) {
            const FrontView& fc = sd ? f1 : f0;
            const int npc = fc.np, nbc = fc.nf - fc.np;
            const int ra = sd ? ra1 : ra0;                        // -1 beyond the front and where the child is not there
            const unsigned rowb = 8u * (unsigned)(max(ra, npc) - npc);
            bool cok[TS / 4];
#pragma unroll
            for (int k = 0; k < TS / 4; ++k) {
                const int lc = lc0 + 4 * k;
                const int b = __builtin_amdgcn_readfirstlane(cmap[sd][lc]);
                cok[k] = b >= 0 && c0 + lc < c_end;
                const char* cb = reinterpret_cast<const char*>(fc.S + (size_t)nbc * (size_t)(max(b, npc) - npc));
                g[sd][k] = *reinterpret_cast<const double*>(cb + rowb);
            }
#pragma unroll
            for (int k = 0; k < TS / 4; ++k)
                if (!(ra >= 0 && cok[k] && (!diag || c0 + lc0 + 4 * k <= r))) g[sd][k] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < TS / 4; ++k) v[k] = (0.0 + g[0][k]) + g[1][k];      // the sums of the general gather below, term by term
    } else {
#pragma unroll
    for (int k = 0; k < TS / 4; ++k) {
        const int lc = lc0 + 4 * k, cc = c0 + lc;
        double x = 0.0;
        if (r < nfp && cc <= r && cc < c_end) {
            const int b0 = cmap[0][lc], b1 = cmap[1][lc];
            if (ra0 >= 0 && b0 >= 0) x += f0.col(min(ra0, b0))[max(ra0, b0)];
            if (ra1 >= 0 && b1 >= 0) x += f1.col(min(ra1, b1))[max(ra1, b1)];
        }
        v[k] = x;
    }
    }
#pragma unroll
    for (int k = 0; k < TS / 4; ++k) {
        const int cc = c0 + lc0 + 4 * k;
        if (r < nfp && cc <= r && cc < c_end) {
            double x = v[k];
            if (mask && r == cc && r < npp && mask[gd[r]]) x = 1.0;
            fp.col(cc)[r] = x;
        }
    }
}

// ------------------------------------------------------------------------------------------ factorisation
// Cholesky of a 32x32 block and the inverse of its factor, in the registers of one wave.
// Lanes 0..31 own the rows of the block, lanes 32..63 the columns of an identity: running the same
// elimination on both halves (A = L L^T on the left, L X = I on the right) yields the factor and its inverse
// from one instruction stream -- the multipliers L[c][j] are the same for both.
// On entry a[] = row `lane` of the block (lanes < 32) or column `lane - 32` of the identity (lanes >= 32);
// on return lane r < 32 holds row r of L, lane 32 + c holds column c of L^-1 (a[r] = Linv[r][c]).
// Pivots and multipliers travel by v_readlane (static lane ids).
// Returns the number of non-positive pivots that had to be repaired.
// broadcast of a double from a compile-time lane: two v_readlane_b32 (a 64-wide __shfl here sends hipcc's
// optimiser into a compile that does not finish within minutes once the loops below are unrolled)
__device__ __forceinline__ double rl(double v, int lane) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, lane);
    hi = __builtin_amdgcn_readlane(hi, lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double rsqrt_newton(double d) {
    // 1/sqrt(d): hardware estimate + two Newton steps (no fp64 sqrt / divide expansion on the critical path)
    double y = __builtin_amdgcn_rsq(d);
    double e = 1.0 - d * y * y;
    y = y + 0.5 * y * e;
    e = 1.0 - d * y * y;
    y = y + 0.5 * y * e;
    return y;
}

// W = width of the block (32: lanes 0..31 rows, 32..63 identity columns; 16: lanes 0..15 rows, 16..31 identity columns, and
// whatever rows lanes 32.. carry receive the same column operations, i.e. become rows of L21 = A21 L11^-T for free).
template <int W>
__device__ __forceinline__ int chol_inverse_w(double (&a)[W], int wb, int lane) {
    int bad = 0;
    // pivot of step 0
    double d = rl(a[0], 0);
    if (!(d > 0.0)) { if (0 < wb) bad += 1; d = fabs(d) > 1e-300 ? fabs(d) : 1.0; }
    double y = rsqrt_newton(d);
#pragma unroll
    for (int j = 0; j < W; ++j) {
        // left half: column j of L for this lane's row (valid for lane >= j); right half: row j of L^-1
        const double l = (lane == j) ? d * y : a[j] * y;
        a[j] = l;
        if (j + 1 < W) {
            // the next pivot is final after the first update: start its reciprocal square root now, so that this
            // dependent chain (~150 cycles) runs beside the remaining updates of this step instead of after them
            a[j + 1] -= l * rl(l, j + 1);
            asm volatile("" : "+v"(a[j + 1]));
            d = rl(a[j + 1], j + 1);
            if (j + 1 < wb) {
                if (!(d > 0.0)) { bad += 1; d = fabs(d) > 1e-300 ? fabs(d) : 1.0; }
            } else {
                d = 1.0;
            }
            y = rsqrt_newton(d);
        }
#pragma unroll
        for (int c = j + 2; c < W; c += 2) {
            // two broadcasts ahead of two updates: no wait states between a v_readlane and the FMA that consumes it
            const double lc0 = rl(l, c);                      // L[c][j]
            const double lc1 = (c + 1 < W) ? rl(l, c + 1) : 0.0;
            a[c] -= l * lc0;                                  // left half: only entries with c <= row are meaningful
            if (c + 1 < W) a[c + 1] -= l * lc1;
            // pin the updates to this step: a[c] is not consumed before step c, and left to itself the compiler
            // defers the FMAs until then, keeping every broadcast alive in SGPRs (1500 of them spilled)
            asm volatile("" : "+v"(a[c]));
            if (c + 1 < W) asm volatile("" : "+v"(a[c + 1]));
        }
    }
    return bad;
}

__device__ __forceinline__ int chol32_inverse(double (&a)[NB], int wb, int lane) { return chol_inverse_w<NB>(a, wb, lane); }

// The same factor + inverse without a square root on the critical path: A = L~ D L~^T (unit lower L~), one pivot per step.
// The register elimination above spends ~500 cycles per step, most of them waiting: pivot -> rsq + two Newton steps -> scale
// the column -> broadcast -> update the next diagonal entry -> broadcast it -> next pivot, a chain of ~20 dependent
// instructions.  Here the next pivot is formed on the scalar side,  d' = A[j+1][j+1] - A[j+1][j]^2 / d,  from two broadcasts
// that do not wait for this step (both entries were final one step earlier): the chain is  d -> rcp + two Newton steps -> one
// FMA -> d',  and everything else -- the multipliers m = a[j] / d, their broadcasts, the updates a[c] -= a[j] m_c -- hangs off
// it instead of sitting on it.  Left lanes (rows of A) and right lanes (columns of the identity, i.e. the forward
// substitution z = L~^-1 e_k) run the same instruction stream, as above.
// On return: lane 32 + k holds z (a[r] = (L~^-1)[r][k]); *rs = 1 / sqrt(d_lane) for lanes < 32, so that the inverse of the
// Cholesky factor L = L~ D^1/2 is  X[r][k] = rs_r a[r].  REPAIR: non-positive pivots are replaced on the chain (option
// "allow_pivot_repair"); otherwise they are only counted -- the factorisation fails anyway.
__device__ __forceinline__ double rcp_newton(double d) {
    double y = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-d, y, 1.0);
    y = __builtin_fma(y, e, y);
    return y;
}

// Width W as in chol_inverse_w: W = 16 leaves lanes 32.. free to carry rows below the block (they become L~21 D).
template <int W, bool REPAIR>
__device__ __forceinline__ int ldl_inverse_w(double (&a)[W], int wb, int lane, double* rs) {
    int bad = 0;
    double dvec = 1.0;                              // lane j keeps the pivot d_j
    double d = rl(a[0], 0);
    if (REPAIR && !(d > 0.0)) { if (0 < wb) bad += 1; d = fabs(d) > 1e-300 ? fabs(d) : 1.0; }
#pragma unroll
    for (int j = 0; j < W; ++j) {
        dvec = (lane == j) ? d : dvec;
        const double r = rcp_newton(d);
        if (j + 1 < W) {
            const double s = rl(a[j], j + 1), s2 = rl(a[j + 1], j + 1);
            d = __builtin_fma(-(s * s), r, s2);
            if (REPAIR && !(d > 0.0)) { if (j + 1 < wb) bad += 1; d = fabs(d) > 1e-300 ? fabs(d) : 1.0; }
        }
        const double m = a[j] * r;                  // left lanes: L~[row][j]
#pragma unroll
        for (int c = j + 1; c < W; c += 2) {
            const double m0 = rl(m, c);
            const double m1 = (c + 1 < W) ? rl(m, c + 1) : 0.0;
            a[c] -= a[j] * m0;
            if (c + 1 < W) a[c + 1] -= a[j] * m1;
            asm volatile("" : "+v"(a[c]));
            if (c + 1 < W) asm volatile("" : "+v"(a[c + 1]));
        }
    }
    if (!REPAIR) bad = __popcll(__ballot(lane < wb && !(dvec > 0.0)));
    *rs = rsqrt_newton(lane < W ? dvec : 1.0);
    return bad;
}

template <bool REPAIR>
__device__ __forceinline__ int ldl32_inverse(double (&a)[NB], int wb, int lane, double* rs) { return ldl_inverse_w<NB, REPAIR>(a, wb, lane, rs); }

// ldl32_inverse with the multipliers of a step broadcast through LDS: a wave issues one instruction per ~4 cycles whatever its
// kind, and the register broadcast costs two v_readlane_b32 per (step, column) on top of the FMA.  Here every lane stores its
// multiplier once (ds_write_b64) and the updates read m_c back from wave-uniform addresses, two columns per ds_read -- 1.5
// instead of 3 instructions per pair.  The round trip through LDS does not touch the pivot chain (see above), and the one
// update that feeds the NEXT step's multipliers, column j + 1, keeps the register broadcast.  All reads of a step are issued
// before its first FMA (one pin per step, not per column: a pin per column made every read wait for its own latency --
// the round-2 LDS variant of the Cholesky elimination was 2.7 x slower than the register one for that reason).
// `bc`: 64 doubles of LDS owned by the calling wave.
template <bool REPAIR>
__device__ __forceinline__ int ldl32_inverse_lds(double (&a)[NB], int wb, int lane, double* rs, double* bc) {
    int bad = 0;
    double dvec = 1.0;
    double d = rl(a[0], 0);
    if (REPAIR && !(d > 0.0)) { if (0 < wb) bad += 1; d = fabs(d) > 1e-300 ? fabs(d) : 1.0; }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        dvec = (lane == j) ? d : dvec;
        const double r = rcp_newton(d);
        if (j + 1 < NB) {
            const double s = rl(a[j], j + 1), s2 = rl(a[j + 1], j + 1);
            d = __builtin_fma(-(s * s), r, s2);
            if (REPAIR && !(d > 0.0)) { if (j + 1 < wb) bad += 1; d = fabs(d) > 1e-300 ? fabs(d) : 1.0; }
        }
        const double m = a[j] * r;
        if (j + 2 < NB) bc[lane] = m;
        if (j + 1 < NB) a[j + 1] -= a[j] * rl(m, j + 1);
        if (j + 2 < NB) {
            double mc[NB];
#pragma unroll
            for (int c = j + 2; c < NB; ++c) mc[c] = bc[c];
#pragma unroll
            for (int c = j + 2; c < NB; ++c) a[c] -= a[j] * mc[c];
        }
        // pin the whole step: left to itself the compiler defers updates to the step that consumes them
#pragma unroll
        for (int c = j + 1; c < NB; ++c) asm volatile("" : "+v"(a[c]));
    }
    if (!REPAIR) bad = __popcll(__ballot(lane < wb && !(dvec > 0.0)));
    *rs = rsqrt_newton(lane < NB ? dvec : 1.0);
    return bad;
}

// ---- outer panel of <= 128 columns in two launches ----------------------------------------------------------
// 16x16 MFMA sub-block product helpers: wave w of a 4-wave workgroup owns sub-block (w & 1, w >> 1) of a 32x32
// result.  v_mfma_f64_16x16x4_f64: a lane supplies A[i = lane & 15][k = lane >> 4] and B[k = lane >> 4][j = lane & 15]
// and holds D[i = (lane >> 4) + 4 reg][j = lane & 15].
typedef double mfma_d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));
typedef double blk32[NB][NB + 1];

// acc += A(32 x 32) * B(32 x 32) restricted to this wave's sub-block; TA / TB: the operand is stored transposed
template <bool TA, bool TB>
__device__ __forceinline__ void mfma_blk(mfma_d4& acc, const blk32& A, const blk32& B, int si, int sj, int l15, int l4) {
#pragma unroll
    for (int kk = 0; kk < NB; kk += 4) {
        const double a = TA ? A[kk + l4][16 * si + l15] : A[16 * si + l15][kk + l4];
        const double b = TB ? B[16 * sj + l15][kk + l4] : B[kk + l4][16 * sj + l15];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
}

// One wave: acc += M1 (16 x 16) M2 (16 x 16), both row-major in LDS with leading dimension LDB = NB + 1 (quadrants of a blk32).
// NEG1: the first operand enters negated.  TB: M2 is stored transposed (the product is M1 M2^T).
template <bool NEG1, bool TB>
__device__ __forceinline__ void mm16(mfma_d4& acc, const double* M1, const double* M2, int l15, int l4) {
#pragma unroll
    for (int kk = 0; kk < 16; kk += 4) {
        const double a = M1[l15 * (NB + 1) + kk + l4];
        const double b = TB ? M2[l15 * (NB + 1) + kk + l4] : M2[(kk + l4) * (NB + 1) + l15];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(NEG1 ? -a : a, b, acc, 0, 0, 0);
    }
}

// The inverse of the Cholesky factor of the 32 x 32 block B (lower triangle valid, in LDS), by ONE wave, in place: on return
// B holds X = L^-1 (lower triangle, zeros above).  Two register factorisations of 16 columns instead of one of 32 -- a step of
// the register elimination costs its pivot chain (~110 cycles) plus three instructions per remaining column, and half of the
// columns halve that -- with the 16 x 16 glue on the matrix cores, staged through the free quadrants of B itself:
//   A  lanes 0..15 rows of B11, 16..31 identity, 32..47 rows of B21:  L11, X11 = L11^-1, L21 = B21 L11^-T     (registers)
//   B  B22 -= L21 L21^T                                                                                       (MFMA)
//   C  lanes 0..15 rows of B22, 16..31 identity:  L22, X22                                                    (registers)
//   D  X21 = -X22 (L21 X11)                                                                                   (MFMA)
// LDS operations of one wave execute in order, so the phases need no barrier.  Returns the number of repaired pivots.
template <bool LDL, bool REPAIR>
__device__ __forceinline__ int chol32_inverse_v2(blk32& B, int wb, int lane) {
    constexpr int H = NB / 2, LDB = NB + 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    double* b00 = &B[0][0];
    double* b01 = b00 + H;                  // upper-right quadrant: scratch for L21 (zeroed at the end)
    double* b10 = b00 + H * LDB;            // B21, then T = L21 X11, then X21
    double* b11 = b10 + H;                  // B22, then X22
    double a[H];
    {
        const int grp = lane >> 4;          // 0 rows of B11, 1 identity, 2 rows of B21, 3 unused
        const double* src = grp == 2 ? b10 + l15 * LDB : b00 + l15 * LDB;
#pragma unroll
        for (int c = 0; c < H; ++c) {
            const double v = src[c];
            a[c] = (grp == 1) ? (c == l15 ? 1.0 : 0.0) : (grp == 3 ? 0.0 : v);
        }
    }
    int bad;
    if (LDL) {
        // LDL^T elimination (no square root on the pivot chain), then L = L~ D^1/2: columns of the left rows (lanes 0..15 and
        // 32..47: a[k] = L~[.][k] d_k) and rows of the inverse (lanes 16..31: a[r] = (L~^-1)[r][.]) take the same factor rs_i
        double rs;
        bad = ldl_inverse_w<H, REPAIR>(a, min(wb, H), lane, &rs);
#pragma unroll
        for (int i = 0; i < H; ++i) a[i] *= rl(rs, i);
    } else {
        bad = chol_inverse_w<H>(a, min(wb, H), lane);
    }
    // X11 into place (lane 16 + c holds its column c), L21 into the scratch quadrant (lane 32 + i holds its row i)
    if (l4 == 1) {
#pragma unroll
        for (int r = 0; r < H; ++r) b00[r * LDB + l15] = (r >= l15 && r < wb && l15 < wb) ? a[r] : 0.0;
    } else if (l4 == 2) {
#pragma unroll
        for (int k = 0; k < H; ++k) b01[l15 * LDB + k] = a[k];
    }
    __builtin_amdgcn_wave_barrier();
    {   // B22 -= L21 L21^T (upper triangle: garbage in, garbage out -- never read)
        mfma_d4 acc;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) acc[reg] = b11[(l4 + 4 * reg) * LDB + l15];
        mm16<true, true>(acc, b01, b01, l15, l4);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) b11[(l4 + 4 * reg) * LDB + l15] = acc[reg];
    }
    __builtin_amdgcn_wave_barrier();
    {
        const double* src = b11 + l15 * LDB;
#pragma unroll
        for (int c = 0; c < H; ++c) {
            const double v = src[c];
            a[c] = (l4 == 1) ? (c == l15 ? 1.0 : 0.0) : (l4 == 0 ? v : 0.0);
        }
    }
    const int wb2 = max(wb - H, 0);
    if (LDL) {
        double rs;
        bad += ldl_inverse_w<H, REPAIR>(a, wb2, lane, &rs);
#pragma unroll
        for (int i = 0; i < H; ++i) a[i] *= rl(rs, i);
    } else {
        bad += chol_inverse_w<H>(a, wb2, lane);
    }
    if (l4 == 1) {
#pragma unroll
        for (int r = 0; r < H; ++r) b11[r * LDB + l15] = (r >= l15 && r < wb2 && l15 < wb2) ? a[r] : 0.0;
    }
    __builtin_amdgcn_wave_barrier();
    {   // T = L21 X11 -> b10;  X21 = -X22 T -> b10
        mfma_d4 t = (mfma_d4){0.0, 0.0, 0.0, 0.0};
        mm16<false, false>(t, b01, b00, l15, l4);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) b10[(l4 + 4 * reg) * LDB + l15] = t[reg];
        __builtin_amdgcn_wave_barrier();
        mfma_d4 x = (mfma_d4){0.0, 0.0, 0.0, 0.0};
        mm16<true, false>(x, b11, b10, l15, l4);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            b10[(l4 + 4 * reg) * LDB + l15] = x[reg];
            b01[(l4 + 4 * reg) * LDB + l15] = 0.0;
        }
    }
    __builtin_amdgcn_wave_barrier();
    return bad;
}

// PA: the diagonal block [C0, C0+kw) x [C0, C0+kw), kw <= 128, of every front of the level -- one workgroup per front.
// The block is held in LDS as 32x32 sub-blocks (lower block triangle).  For each block column j: wave 0 factorises
// the diagonal sub-block and inverts its factor in registers (chol32_inverse); the four waves then form
// L_ij = D_ij Linv_j^T and D_ik -= L_ij L_kj^T on the matrix cores.  Afterwards the inverse S of the whole kw x kw
// factor is accumulated block-wise (S_jj = Linv_j, S_ij = -Linv_i sum_{k=j}^{i-1} L_ik S_kj) and stored
// column-major with leading dimension 128: k_panel_rows turns the rows below the block into factor rows with one
// GEMM against S^T, and the wide triangular solves use the same S.
// Outputs: off-diagonal sub-blocks of L into F, the 32x32 inverses into Linv, S into Sout.
// The diagonal sub-blocks of F are left as they were (nothing reads them afterwards).
#ifdef FEMO_PANEL_STAMPS
__device__ long long g_stamps[32];
#define STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_stamps[i] = wall_clock64(); } while (0)
#else
#define STAMP(i)
#endif

// LDS is sized by the launch: `nblk` = the largest number of 32-column sub-blocks any front of the launch has in this
// panel (the host sorts the fronts of a level by pivot count and launches them in classes), so that the many small
// fronts at the bottom of the tree run two or three workgroups per CU instead of one.
// r3: the inverse needs no LDS of its own -- column j of S and the scratch block of a product live in the sub-blocks of L's
// column j, each of which is dead once its row's sum has been formed (112 -> 80 KB for four sub-blocks: two workgroups per CU).
__device__ __host__ inline int diag_block_lds_blocks(int nblk) { return nblk * (nblk + 1) / 2; }

// fuse_rows (fronts of ONE panel on levels that do not keep S): the rows below the block are turned into factor rows here, with
// S read from LDS where the inverse phase leaves it -- S never goes to memory and k_panel_rows is not launched.  On the leaves
// this kernel is HBM-bound (block in, factor sub-blocks, the 32 x 32 inverses and the 128 x 128 S out: 2.4 GB at 1 M DOF), and S is
// the largest item; k_panel_rows then read it back.
__global__ void __launch_bounds__(256)
k_diag_block(FrontDev fd, const int* __restrict__ level_nodes, int first, int nblk, int C0, double* __restrict__ Swork,
             int* __restrict__ info, int fuse_rows) {
    STAMP(31);
    const int slot = first + blockIdx.x;                       // position of the front in its level
    const int t = level_nodes[slot];
    const int np = fd.npiv[t];
    if (C0 >= np) return;
    const int kw = min(NBO, np - C0);
    const int nkb = (kw + NB - 1) / NB;
    const int ldp = ldp_of(fd.nf[t]);
    double* F = fd.P + fd.poff[t];                             // pivot columns only
    // the inverse of this diagonal block: scratch (levels solved with the one-workgroup-per-front kernels) or the diagonal
    // block of the front's X (wide levels)
    const int lds_ = Swork ? SPD : ldx_of(np);
    double* Sout = Swork ? Swork + (size_t)slot * SPD * SPD : fd.X + fd.xoff[t] + C0 + (size_t)lds_ * C0;
    extern __shared__ double lds_raw[];
    blk32* D = reinterpret_cast<blk32*>(lds_raw);              // sub-block (i, j), i >= j, at i (i + 1) / 2 + j
    const int nD = nblk * (nblk + 1) / 2;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int si = wv & 1, sj = wv >> 1, l15 = lane & 15, l4 = lane >> 4;
    // load (identity padding beyond kw; only the lower triangle of the front is maintained): all 40 loads of a thread
    // are issued before the first one is consumed -- a loop over the sub-blocks would pay the memory latency ten times
    {
        double v[10][4];
#pragma unroll
        for (int b = 0; b < 10; ++b) {
            const int bi = b < 1 ? 0 : b < 3 ? 1 : b < 6 ? 2 : 3;
            const int bj = b - bi * (bi + 1) / 2;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = tid + 256 * q;
                const int r = idx % NB, c = idx / NB;
                const int gr = NB * bi + r, gc = NB * bj + c;
                v[b][q] = (gr == gc) ? 1.0 : 0.0;
                if (b < nD && bi < nkb && gr < kw && gc < kw && gc <= gr) v[b][q] = F[(C0 + gr) + (size_t)ldp * (C0 + gc)];
            }
        }
#pragma unroll
        for (int b = 0; b < 10; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = tid + 256 * q;
                if (b < nD) D[b][idx % NB][idx / NB] = v[b][q];
            }
    }
    // (no zero fill of S: every sub-block on or below the block diagonal is written in full below, and nothing above it
    //  or beyond the kw columns is ever read)
    STAMP(0);
    __syncthreads();
    STAMP(1);
    for (int j = 0; j < nkb; ++j) {
        blk32& Djj = D[j * (j + 1) / 2 + j];
        const int wb = min(NB, kw - NB * j);
        STAMP(2 + 4 * j);
        if (wv == 0) {
            double a[NB];
#pragma unroll
            for (int c = 0; c < NB; ++c) a[c] = (lane < NB) ? Djj[lane][c] : (c == lane - NB ? 1.0 : 0.0);
            const int bad = chol32_inverse(a, wb, lane);
            if (lane >= NB) {
                const int cl = lane - NB;               // this lane holds column cl of the inverse
                double* Li = fd.Linv + fd.linvoff[t] + (size_t)(C0 / NB + j) * NB * NB;
#pragma unroll
                for (int r = 0; r < NB; ++r) {
                    const double v = (cl < wb && r < wb && cl <= r) ? a[r] : 0.0;
                    Djj[r][cl] = v;                     // the diagonal sub-block now holds Linv_j
                    Li[r + NB * cl] = v;
                }
                if (cl == 0 && bad) atomicAdd(info, bad);
            }
        }
        __syncthreads();
        STAMP(3 + 4 * j);
        if (j + 1 < nkb) {
            // L_ij = D_ij Linv_j^T for the sub-blocks below
            mfma_d4 acc[3];
#pragma unroll
            for (int i = 1; i < 4; ++i) {
                acc[i - 1] = (mfma_d4){0.0, 0.0, 0.0, 0.0};
                if (j + i < nkb) mfma_blk<false, true>(acc[i - 1], D[(j + i) * (j + i + 1) / 2 + j], Djj, si, sj, l15, l4);
            }
            __syncthreads();
#pragma unroll
            for (int i = 1; i < 4; ++i) {
                if (j + i >= nkb) continue;
                blk32& Dij = D[(j + i) * (j + i + 1) / 2 + j];
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int r = 16 * si + l4 + 4 * reg, c = 16 * sj + l15;
                    Dij[r][c] = acc[i - 1][reg];
                    const int gr = NB * (j + i) + r, gc = NB * j + c;
                    if (gr < kw && gc < kw) F[(C0 + gr) + (size_t)ldp * (C0 + gc)] = acc[i - 1][reg];
                }
            }
            __syncthreads();
            STAMP(4 + 4 * j);
            // D_ik -= L_ij L_kj^T, i >= k > j (each wave updates its own sub-block of every D_ik)
            for (int i = j + 1; i < nkb; ++i)
                for (int k = j + 1; k <= i; ++k) {
                    mfma_d4 u = (mfma_d4){0.0, 0.0, 0.0, 0.0};
                    mfma_blk<false, true>(u, D[i * (i + 1) / 2 + j], D[k * (k + 1) / 2 + j], si, sj, l15, l4);
                    blk32& Dik = D[i * (i + 1) / 2 + k];
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) Dik[16 * si + l4 + 4 * reg][16 * sj + l15] -= u[reg];
                }
            __syncthreads();
        }
    }
    // inverse of the kw x kw factor, block column by block column
    STAMP(20);
    for (int j = 0; j < nkb; ++j) {
        const blk32& Sjj = D[j * (j + 1) / 2 + j];
        if (!fuse_rows)
        for (int idx = tid; idx < NB * NB; idx += 256) {
            const int r = idx % NB, c = idx / NB;
            Sout[(NB * j + r) + (size_t)lds_ * (NB * j + c)] = Sjj[r][c];
        }
        for (int i = j + 1; i < nkb; ++i) {
            // W = sum_{k=j}^{i-1} L_ik S_kj: S_kj (j < k < i) already sits where L_kj was; L_ij is read here for the last time
            blk32& Dij = D[i * (i + 1) / 2 + j];
            mfma_d4 w = (mfma_d4){0.0, 0.0, 0.0, 0.0};
            for (int k = j; k < i; ++k)
                mfma_blk<false, false>(w, D[i * (i + 1) / 2 + k], D[k * (k + 1) / 2 + j], si, sj, l15, l4);
            __syncthreads();                                   // every wave has read L_ij: its sub-block takes W
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) Dij[16 * si + l4 + 4 * reg][16 * sj + l15] = w[reg];
            __syncthreads();
            // S_ij = -Linv_i W
            mfma_d4 x = (mfma_d4){0.0, 0.0, 0.0, 0.0};
            mfma_blk<false, false>(x, D[i * (i + 1) / 2 + i], Dij, si, sj, l15, l4);
            __syncthreads();                                   // every wave has read W: the sub-block takes S_ij
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int r = 16 * si + l4 + 4 * reg, c = 16 * sj + l15;
                Dij[r][c] = -x[reg];
                if (!fuse_rows) Sout[(NB * i + r) + (size_t)lds_ * (NB * j + c)] = -x[reg];
            }
            __syncthreads();
        }
    }
    STAMP(21);
    if (fuse_rows) {
        // L[r][C0 + c] = sum_{k <= c} A[r][C0 + k] S[c][k] for the rows below the block (k_panel_rows' product): a wave takes 16 rows
        // at a time, their kw entries in registers as the MFMA B operand, S[c][k] from the sub-blocks in LDS as the A operand
        __syncthreads();
        const int nf = fd.nf[t];
        for (int row0 = C0 + kw + 16 * wv; row0 < nf; row0 += 64) {
            const int row = row0 + l15;
            const bool rok = row < nf;
            double a[NBO / 4];
#pragma unroll
            for (int kk = 0; kk < NBO / 4; ++kk) {
                const int k = 4 * kk + l4;
                a[kk] = (rok && k < kw) ? F[row + (size_t)ldp * (C0 + k)] : 0.0;
            }
#pragma unroll
            for (int cb = 0; cb < NBO / 16; ++cb) {
                if (16 * cb >= kw) break;
                const int bi = cb >> 1;
                mfma_d4 acc = (mfma_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int kk = 0; kk < 4 * cb + 4; ++kk)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(D[bi * (bi + 1) / 2 + (kk >> 3)][16 * (cb & 1) + l15][4 * (kk & 7) + l4], a[kk], acc, 0, 0, 0);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int c = 16 * cb + l4 + 4 * reg;
                    if (rok && c < kw) F[row + (size_t)ldp * (C0 + c)] = acc[reg];
                }
            }
        }
    }
}


// ---- k_diag_block2: the same block, the same outputs, scheduled for latency.
// k_diag_block runs its phases one after the other on ONE workgroup: four register factorisations on wave 0 (three waves
// idle), then the MFMA phases with wave 0 idle in between, then the inverse S -- 45 us per block, and the chain of these
// blocks IS the factorisation time at the top of the tree (0.018 of fp64 peak).  Here:
//   * the 32 x 32 factor + inverse is the LDL^T elimination (ldl32_inverse: no square root on the pivot chain);
//   * while wave 0 factorises D_jj, waves 1..3 work through whole 32 x 32 x 32 block products that do not depend on it:
//     the rank-32 updates of the previous block column that the NEXT factorisation does not need, and the rows of the inverse
//     S that are already determined;
//   * between two factorisations only what the next one needs runs on all four waves (by 16 x 16 quadrant): the block column
//     L_ij = D_ij Linv_j^T and the update of D_(j+1)(j+1);
//   * after the last factorisation one product per remaining block of S.
// LDS: D (lower block triangle), the off-diagonal blocks of S, one scratch block per wave 1..3.
__device__ __host__ inline int diag_block2_lds_blocks(int nblk) { return nblk * (nblk + 1) / 2 + nblk * (nblk - 1) / 2 + (nblk > 1 ? 3 : 0); }

// acc (2 x 2 quadrants, D layout) += A B for whole 32 x 32 blocks, one wave
template <bool TA, bool TB>
__device__ __forceinline__ void wave_mm(mfma_d4 (&acc)[2][2], const blk32& A, const blk32& B, int l15, int l4) {
#pragma unroll
    for (int kk = 0; kk < NB; kk += 4) {
        const double a0 = TA ? A[kk + l4][l15] : A[l15][kk + l4], a1 = TA ? A[kk + l4][16 + l15] : A[16 + l15][kk + l4];
        const double b0 = TB ? B[l15][kk + l4] : B[kk + l4][l15], b1 = TB ? B[16 + l15][kk + l4] : B[kk + l4][16 + l15];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
}
__device__ __forceinline__ void wave_zero(mfma_d4 (&acc)[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (mfma_d4){0.0, 0.0, 0.0, 0.0};
}
// block (LDS) = sign * acc, and optionally the same values to global memory (column-major, leading dimension ldg)
template <bool NEG, bool SUB>
__device__ __forceinline__ void wave_store(blk32& dst, const mfma_d4 (&acc)[2][2], int l15, int l4, double* g = nullptr, size_t ldg = 0) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int r = 16 * a + l4 + 4 * reg, c = 16 * b + l15;
                const double v = NEG ? -acc[a][b][reg] : acc[a][b][reg];
                if (SUB) dst[r][c] -= v; else dst[r][c] = v;
                if (g) g[r + ldg * c] = v;
            }
}

template <bool REPAIR>
__global__ void __launch_bounds__(256)
k_diag_block2(FrontDev fd, const int* __restrict__ level_nodes, int first, int nblk, int C0, double* __restrict__ Swork,
              int* __restrict__ info) {
    STAMP(31);
    const int slot = first + blockIdx.x;
    const int t = level_nodes[slot];
    const int np = fd.npiv[t];
    if (C0 >= np) return;
    const int kw = min(NBO, np - C0);
    const int nkb = (kw + NB - 1) / NB;
    const int ldp = ldp_of(fd.nf[t]);
    double* F = fd.P + fd.poff[t];
    const int lds_ = Swork ? SPD : ldx_of(np);
    double* Sout = Swork ? Swork + (size_t)slot * SPD * SPD : fd.X + fd.xoff[t] + C0 + (size_t)lds_ * C0;
    extern __shared__ double lds_raw[];
    const int nD = nblk * (nblk + 1) / 2;
    blk32* D = reinterpret_cast<blk32*>(lds_raw);              // D_ij, i >= j, at i (i + 1) / 2 + j; D_jj becomes Linv_j = S_jj
    blk32* Sb = D + nD;                                         // S_ij, i > j, at i (i - 1) / 2 + j
    blk32* Sc = Sb + nblk * (nblk - 1) / 2;                      // scratch block of wave w at Sc[w - 1]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int si = wv & 1, sj = wv >> 1, l15 = lane & 15, l4 = lane >> 4;
#define DB(i, j) D[(i) * ((i) + 1) / 2 + (j)]
#define SB(i, j) Sb[(i) * ((i) - 1) / 2 + (j)]
#define SOUT(i, j) (Sout + NB * (i) + (size_t)lds_ * (NB * (j)))
    // Load, identity padding beyond kw.  D_00 is needed by the first factorisation only: wave 0 reads its rows straight
    // into registers and factorises them while the other blocks are still on their way to LDS (nobody else touches D[0]).
    double a0[NB];
    if (wv == 0) {
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            a0[c] = (lane < NB) ? (lane == c ? 1.0 : 0.0) : (c == lane - NB ? 1.0 : 0.0);
            if (lane < NB && c <= lane && lane < kw) a0[c] = F[(C0 + lane) + (size_t)ldp * (C0 + c)];
        }
    }
    if (wv > 0) {
        // the other nine blocks: waves 1..3, 192 threads, all loads of a thread in flight before the first store
        constexpr int NL = (9 * NB * NB + 191) / 192;           // 48
        const int t3 = tid - 64;
        double v[NL];
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            const int e = t3 + 192 * q;
            const int b = 1 + e / (NB * NB), idx = e % (NB * NB);
            const int bi = b < 3 ? 1 : b < 6 ? 2 : 3;
            const int bj = b - bi * (bi + 1) / 2;
            const int r = idx % NB, c = idx / NB;
            const int gr = NB * bi + r, gc = NB * bj + c;
            v[q] = (gr == gc) ? 1.0 : 0.0;
            if (b < nD && bi < nkb && gr < kw && gc < kw && gc <= gr) v[q] = F[(C0 + gr) + (size_t)ldp * (C0 + gc)];
        }
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            const int e = t3 + 192 * q;
            const int b = 1 + e / (NB * NB), idx = e % (NB * NB);
            if (b < nD) D[b][idx % NB][idx / NB] = v[q];
        }
    }
    STAMP(0);
    // block tasks of one wave.  L_ij (in place of D_ij) also goes to the front's factor columns.
    auto factor_rows = [&](int i, int j) {                       // T(i, j): D_ij <- L_ij = D_ij Linv_j^T
        mfma_d4 acc[2][2];
        wave_zero(acc);
        wave_mm<false, true>(acc, DB(i, j), DB(j, j), l15, l4);
        blk32& Dij = DB(i, j);
#pragma unroll
        for (int qa = 0; qa < 2; ++qa)
#pragma unroll
            for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int r = 16 * qa + l4 + 4 * reg, c = 16 * qb + l15;
                    Dij[r][c] = acc[qa][qb][reg];
                    const int gr = NB * i + r, gc = NB * j + c;
                    if (gr < kw && gc < kw) F[(C0 + gr) + (size_t)ldp * (C0 + gc)] = acc[qa][qb][reg];
                }
        __builtin_amdgcn_wave_barrier();
    };
    auto update = [&](int i, int k, int j) {                    // U(i, k; j): D_ik -= L_ij L_kj^T
        mfma_d4 acc[2][2];
        wave_zero(acc);
        wave_mm<false, true>(acc, DB(i, j), DB(k, j), l15, l4);
        wave_store<false, true>(DB(i, k), acc, l15, l4);
        __builtin_amdgcn_wave_barrier();
    };
    auto s_block = [&](int i, int j, blk32& W) {                // S_ij = -Linv_i W  -> LDS and global
        mfma_d4 acc[2][2];
        wave_zero(acc);
        wave_mm<false, false>(acc, DB(i, i), W, l15, l4);
        wave_store<true, false>(SB(i, j), acc, l15, l4, SOUT(i, j), (size_t)lds_);
        __builtin_amdgcn_wave_barrier();
    };
    auto s_of = [&](int k, int j) -> const blk32& { return k == j ? DB(j, j) : SB(k, j); };
    auto w_block = [&](int i, int j, blk32& W) {                // W = sum_{k=j}^{i-1} L_ik S_kj
        mfma_d4 acc[2][2];
        wave_zero(acc);
        for (int k = j; k < i; ++k) wave_mm<false, false>(acc, DB(i, k), s_of(k, j), l15, l4);
        wave_store<false, false>(W, acc, l15, l4);
        __builtin_amdgcn_wave_barrier();
    };
    const int last = nkb - 1;
    for (int j = 0; j < nkb; ++j) {
        STAMP(2 + 4 * j);
        if (wv == 0) {
            // ---- F(j): factor + inverse of D_jj in registers; Linv_j replaces D_jj and goes to Linv
            blk32& Djj = DB(j, j);
            const int wb = min(NB, kw - NB * j);
            double a[NB];
#pragma unroll
            for (int c = 0; c < NB; ++c) a[c] = j == 0 ? a0[c] : ((lane < NB) ? Djj[lane][c] : (c == lane - NB ? 1.0 : 0.0));
            double rs;
            const int bad = ldl32_inverse<REPAIR>(a, wb, lane, &rs);
            // rows of the inverse take 1 / sqrt(d_row): the broadcast reads lanes < 32 and must stay outside the divergent store
#pragma unroll
            for (int r = 0; r < NB; ++r) a[r] *= rl(rs, r);
            if (lane >= NB) {
                const int cl = lane - NB;
                double* Li = fd.Linv + fd.linvoff[t] + (size_t)(C0 / NB + j) * NB * NB;
#pragma unroll
                for (int r = 0; r < NB; ++r) {
                    const double v = (cl < wb && r < wb && cl <= r) ? a[r] : 0.0;
                    Djj[r][cl] = v;
                    Li[r + NB * cl] = v;
                }
                if (cl == 0 && bad) atomicAdd(info, bad);
            }
        } else if (j == 1) {
            // ---- beside F(1): block column 0 below row 1 -- its factor rows and the updates they feed.  U(3, 2; 0) needs the
            // rows of both waves and waits for the next stage (D_32 is first read between F(2) and F(3)).
            if (wv == 1 && nkb > 2) { factor_rows(2, 0); update(2, 1, 0); update(2, 2, 0); }
            if (wv == 3 && nkb > 3) { factor_rows(3, 0); update(3, 1, 0); update(3, 3, 0); }
            if (nkb == 2 && wv == 2) w_block(1, 0, Sc[1]);      // last row: W_10 = L_10 S_00
        } else if (j == 2) {
            if (wv == 1 && nkb > 3) { factor_rows(3, 1); update(3, 2, 0); update(3, 2, 1); update(3, 3, 1); }
            if (wv == 3) {                                      // row 1 of S; and the last row's W if this is the last stage
                w_block(1, 0, Sc[2]);
                s_block(1, 0, Sc[2]);
                if (nkb == 3) w_block(2, 0, Sc[2]);             // W_20 = L_20 S_00 + L_21 S_10
            }
            if (nkb == 3 && wv == 2) w_block(2, 1, Sc[1]);      // W_21 = L_21 S_11
        } else if (j == 3) {
            if (wv == 1) { w_block(2, 0, Sc[0]); s_block(2, 0, Sc[0]); w_block(3, 0, Sc[0]); }
            if (wv == 2) { w_block(2, 1, Sc[1]); s_block(2, 1, Sc[1]); w_block(3, 1, Sc[1]); }
            if (wv == 3) { w_block(3, 2, Sc[2]); }
        }
        __syncthreads();
        STAMP(3 + 4 * j);
        {   // S_jj = Linv_j to its place (all threads; stores only)
            const blk32& Sjj = DB(j, j);
            for (int idx = tid; idx < NB * NB; idx += 256) {
                const int r = idx % NB, c = idx / NB;
                SOUT(j, j)[r + (size_t)lds_ * c] = Sjj[r][c];
            }
        }
        if (j + 1 < nkb) {
            // ---- between two factorisations, on all four waves by quadrant: only what F(j + 1) needs --
            // L_(j+1)j = D_(j+1)j Linv_j^T, then D_(j+1)(j+1) -= L_(j+1)j L_(j+1)j^T
            mfma_d4 acc = (mfma_d4){0.0, 0.0, 0.0, 0.0};
            mfma_blk<false, true>(acc, DB(j + 1, j), DB(j, j), si, sj, l15, l4);
            __syncthreads();
            {
                blk32& Dij = DB(j + 1, j);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int r = 16 * si + l4 + 4 * reg, c = 16 * sj + l15;
                    Dij[r][c] = acc[reg];
                    const int gr = NB * (j + 1) + r, gc = NB * j + c;
                    if (gr < kw && gc < kw) F[(C0 + gr) + (size_t)ldp * (C0 + gc)] = acc[reg];
                }
            }
            __syncthreads();
            mfma_d4 u = (mfma_d4){0.0, 0.0, 0.0, 0.0};
            mfma_blk<false, true>(u, DB(j + 1, j), DB(j + 1, j), si, sj, l15, l4);
            blk32& Dn = DB(j + 1, j + 1);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) Dn[16 * si + l4 + 4 * reg][16 * sj + l15] -= u[reg];
            __syncthreads();
            STAMP(4 + 4 * j);
        }
    }
    STAMP(20);
    // ---- after the last factorisation: S_(last)(j) = -Linv_last W_(last)(j), by quadrant on all four waves
    int wsrc[3] = {0, 0, 0};                                    // scratch block that holds W_(last)(j)
    if (nkb == 2) wsrc[0] = 1;
    if (nkb == 3) { wsrc[0] = 2; wsrc[1] = 1; }
    if (nkb == 4) { wsrc[0] = 0; wsrc[1] = 1; wsrc[2] = 2; }
    for (int j = 0; j < last; ++j) {
        mfma_d4 x = (mfma_d4){0.0, 0.0, 0.0, 0.0};
        mfma_blk<false, false>(x, DB(last, last), Sc[wsrc[j]], si, sj, l15, l4);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = 16 * si + l4 + 4 * reg, c = 16 * sj + l15;
            SOUT(last, j)[r + (size_t)lds_ * c] = -x[reg];
        }
    }
    STAMP(21);
#undef DB
#undef SB
#undef SOUT
}

// PB: rows below the diagonal block of the outer panel: L[r][C0 + c] = sum_{k <= c} A[r][C0 + k] S[c][k] -- one GEMM
// per 64-row tile against the inverse S of the diagonal block's factor (k_diag_block).  A wave owns 16 rows: their
// kw <= 128 entries sit in registers as the MFMA B operand (read once, so the result can overwrite them in place),
// S streams from L2 as the A operand, and the product is formed transposed so that the stores run along the
// columns of the column-major front.
__global__ void __launch_bounds__(256, 4)      // four waves per SIMD (measured: -15 % against three, 20 B of scratch)
k_panel_rows(FrontDev fd, const int* __restrict__ level_nodes, int first, int C0, const double* __restrict__ Swork) {
    const int slot = first + blockIdx.y;                       // position of the front in its level
    const int t = level_nodes[slot];
    const int np = fd.npiv[t];
    if (C0 >= np) return;
    const int kw = min(NBO, np - C0);
    const int nf = fd.nf[t];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int tile0 = C0 + kw + blockIdx.x * TS;
    if (tile0 >= nf) return;
    const int row0 = tile0 + 16 * wv;
    double* F = fd.P + fd.poff[t];                             // pivot columns only
    const int ldp = ldp_of(nf);
    const int lds_ = Swork ? SPD : ldx_of(np);
    const double* S = Swork ? Swork + (size_t)slot * SPD * SPD : fd.X + fd.xoff[t] + C0 + (size_t)lds_ * C0;
    // S is shared by the four waves: the 16 rows of S that produce output columns [16 cb, 16 cb + 16) are staged in
    // LDS (k-major, so that the MFMA A operand S[c][k] is a conflict-free read), double-buffered over cb
    __shared__ double sb[2][NBO][16];
    const int row = row0 + l15;
    const bool rok = row < nf;
    double a[NBO / 4];
#pragma unroll
    for (int kk = 0; kk < NBO / 4; ++kk) {
        const int k = 4 * kk + l4;
        a[kk] = (rok && k < kw) ? F[row + (size_t)ldp * (C0 + k)] : 0.0;
    }
    const int sc = tid & 15, sk0 = tid >> 4;              // staging: column sc of the block, rows sk0, sk0 + 16, ...
    double pre[NBO / 16];
    // stage block 0
#pragma unroll
    for (int q = 0; q < 1; ++q) pre[q] = S[sc + (size_t)lds_ * (sk0 + 16 * q)];
    sb[0][sk0][sc] = pre[0];
    __syncthreads();
#pragma unroll
    for (int cb = 0; cb < NBO / 16; ++cb) {
        if (16 * cb >= kw) break;
        const int cur = cb & 1;
        const bool more = cb + 1 < NBO / 16 && 16 * (cb + 1) < kw;
        if (more) {
#pragma unroll
            for (int q = 0; q < cb + 2; ++q) pre[q] = S[(16 * (cb + 1) + sc) + (size_t)lds_ * (sk0 + 16 * q)];
        }
        mfma_d4 acc = (mfma_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4 * cb + 4; ++kk)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sb[cur][4 * kk + l4][l15], a[kk], acc, 0, 0, 0);   // D[i = column][j = row]
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int c = 16 * cb + l4 + 4 * reg;
            if (rok && c < kw) F[row + (size_t)ldp * (C0 + c)] = acc[reg];
        }
        if (more) {
#pragma unroll
            for (int q = 0; q < cb + 2; ++q) sb[cur ^ 1][sk0 + 16 * q][sc] = pre[q];
        }
        __syncthreads();
    }
}

// The same product cut finer, for launches that do not fill the chip (the top of the tree: a launch lasts as long as ONE workgroup
// does, and k_panel_rows gives a wave 144 dependent MFMAs behind eight staged loads of S).  A workgroup takes 16 rows; wave w
// forms their output column blocks w and 7 - w (4 w + 4 and 32 - 4 w MFMAs: 36 per wave, a quarter of k_panel_rows' chain).  No
// LDS: the MFMA A operand S[c][k] (16 consecutive c per k: one 128-byte segment) and the rows travel straight to registers, all
// loads of a wave in flight at once.  The product overwrites the rows in place and the four waves share them, so every wave
// has ALL its loads back before any wave stores (the barrier).
__global__ void __launch_bounds__(256, 2)
k_panel_rows_fine(FrontDev fd, const int* __restrict__ level_nodes, int first, int C0, const double* __restrict__ Swork) {
    const int slot = first + blockIdx.y;
    const int t = level_nodes[slot];
    const int np = fd.npiv[t];
    if (C0 >= np) return;                                     // (uniform per workgroup: no barrier is skipped by part of it)
    const int kw = min(NBO, np - C0);
    const int nf = fd.nf[t];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int row0 = C0 + kw + blockIdx.x * 16;
    if (row0 >= nf) return;
    double* F = fd.P + fd.poff[t];
    const int ldp = ldp_of(nf);
    const int lds_ = Swork ? SPD : ldx_of(np);
    const double* S = Swork ? Swork + (size_t)slot * SPD * SPD : fd.X + fd.xoff[t] + C0 + (size_t)lds_ * C0;
    constexpr int NCB = NBO / 16;
    const int ncb = (kw + 15) / 16;
    const int cbs[2] = {wv, NCB - 1 - wv};                    // this wave's two column blocks
    const int row = row0 + l15;
    const bool rok = row < nf;
    double a[NBO / 4];
#pragma unroll
    for (int kk = 0; kk < NBO / 4; ++kk) {
        const int k = 4 * kk + l4;
        a[kk] = (rok && k < kw) ? F[row + (size_t)ldp * (C0 + k)] : 0.0;
    }
    // S operands of both blocks: block cb needs k < 16 cb + 16; the second block (cb >= 4) the longer chain
    double s0[4 * (NCB / 2)], s1[4 * NCB];
#pragma unroll
    for (int kk = 0; kk < 4 * (NCB / 2); ++kk)
        s0[kk] = (cbs[0] < ncb && kk < 4 * cbs[0] + 4) ? S[(16 * cbs[0] + l15) + (size_t)lds_ * (4 * kk + l4)] : 0.0;
#pragma unroll
    for (int kk = 0; kk < 4 * NCB; ++kk)
        s1[kk] = (cbs[1] < ncb && kk < 4 * cbs[1] + 4) ? S[(16 * cbs[1] + l15) + (size_t)lds_ * (4 * kk + l4)] : 0.0;
    mfma_d4 acc0 = (mfma_d4){0.0, 0.0, 0.0, 0.0}, acc1 = (mfma_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 4 * (NCB / 2); ++kk)
        if (kk < 4 * cbs[0] + 4) acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(s0[kk], a[kk], acc0, 0, 0, 0);      // D[i = column][j = row]
#pragma unroll
    for (int kk = 0; kk < 4 * NCB; ++kk)
        if (kk < 4 * cbs[1] + 4) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(s1[kk], a[kk], acc1, 0, 0, 0);
    // every load of this workgroup has been consumed by an MFMA above: the rows may be overwritten once all waves are here
    __syncthreads();
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int c0 = 16 * cbs[0] + l4 + 4 * reg, c1 = 16 * cbs[1] + l4 + 4 * reg;
        if (rok && c0 < kw) F[row + (size_t)ldp * (C0 + c0)] = acc0[reg];
        if (rok && c1 < kw) F[row + (size_t)ldp * (C0 + c1)] = acc1[reg];
    }
}

// P2: rank-k update  C[r][c] -= sum_m L[r][m] L[c][m]  of lower-triangle 64x64 tiles with v_mfma_f64_16x16x4_f64.
// Workgroup = 4 waves = one 64x64 tile of the front; wave w owns the 32x32 quarter (w&1 rows, w>>1 columns) as
// 2x2 MFMA blocks.  To make the stores run along rows of the column-major front (coalesced), the product is
// formed transposed: A[i][k] = L[c0+i][k] (tile columns), B[k][j] = L[r0+j][k] (tile rows), so D[i][j] = C[r0+j][c0+i];
// per the CDNA4 f64 layout a lane holds A[lane&15][lane>>4], B[lane>>4][lane&15] and D[(lane>>4) + 4*reg][lane&15].
// LDS rows are padded to 80 doubles so that the four 16-lane groups of a ds_read_b64 hit disjoint banks.
constexpr int LSTR = TS + 16;

// The K range and the updated columns of one front in one k_trailing_mfma launch (shared with the host's flop count).
//   schur 0  left-looking: the 128 pivot columns at C0 receive the updates of the factor columns [K0, C0) right
//            before they are factorised (K0 = 0: all earlier columns; K0 = start of the super-panel: see below);
//   schur 1  the Schur complement is updated once, after the last panel, with K = npiv.  Every entry of the front is
//            then read and written once per factorisation instead of once per 128 factor columns;
//   schur 2  right-looking: everything behind the factor columns [C0, C0 + KW) is updated with those columns
//            (KW = 128: after every outer panel; KW = 256, 512: after a super-panel whose own panels were updated
//            with schur 0 / K0 = C0 -- the Schur complement then moves through HBM once per KW columns);
//   schur 3, 4  the look-ahead split of 2: only the next 128 columns | everything behind those.
struct TrailRange { int kc0, kw, col_lo, col_hi; };
__device__ __host__ inline TrailRange trail_range(int schur, int C0, int K0, int KW, int np, int nf) {
    TrailRange r{0, 0, 0, 0};
    if (schur != 1 && C0 >= np) return r;
    r.kc0 = schur >= 2 ? C0 : (schur ? 0 : K0);
    r.kw = schur >= 2 ? (KW < np - C0 ? KW : np - C0) : (schur ? np : C0 - K0);
    // the look-ahead split (3 | 4) sits 128 columns behind the even anchor of the first updated column
    const int split = ((C0 + r.kw) & ~1) + NBO;
    r.col_lo = schur >= 2 ? (schur == 4 ? split : C0 + r.kw) : (schur ? np : C0);
    r.col_hi = schur == 0 ? (C0 + NBO < np ? C0 + NBO : np) : schur == 3 ? (split < nf ? split : nf) : nf;
    return r;
}

// ---- the gather of the rank-k updates: what a lane's entries of a not yet existing tile are -- the sum of the entries of the two
// children's Schur complements that land there.  The lane holds NR rows r[b] and NA x 4 columns cc[a][reg] of the front t (the D
// layout of the MFMA blocks of its wave); the launch owns the columns [col_lo, col_hi).  Out: per entry g0 + g1, the left child's
// entry plus the right child's, 0 where a child has none or the entry is not in the lower triangle (r < cc) or outside the front.
// Child rows are boundary rows of the child (>= its pivot count npc), so an entry sits in the child's Schur block
// S_c[(hi - npc) + nbc (lo - npc)], hi >= lo the child rows of the pair.

// Both children land in increasing rows (FrontDev::cmono, child_maps.h): for r >= cc the child rows are ordered as they stand,
// hi = the row's, lo = the column's.  The byte offset of an entry is then a term of the column alone (8 per lane and child) plus
// one of the row alone (NR per lane and child), one 32-bit addition per entry on top of the child's uniform base pointer; whether
// the entry exists is a row predicate AND a column predicate; r >= cc needs testing only in the tiles on the diagonal (DIAG).
// Absent rows and columns are clamped to the first entry of the child's block, so that every address is a valid one, and the value
// is zeroed afterwards.  All of it is integer arithmetic on purpose -- masks of all ones / all zeros made with shifts, applied with
// AND / OR: a select on an address or on a loaded value makes the compiler branch around the load behind a full wait.
// A block of at most 2^14 rows keeps the offsets inside 32 bits (femo_set_frontal_plan clears the flag beyond).
// In two steps, so that a wave of k_trailing_mfma can finish one block row (a) of its tile -- 16 loads, sums, stores -- before it
// fetches the next: all 32 entries of both children in flight beside the 32 accumulator registers do not fit 128 registers.
// The maps are read once, for both block rows, before the first store.
template <int NA, int NR>
struct GatherMono {
    const char* Sc[2];                 // the children's Schur blocks
    unsigned colb[2][NA][4], rowb[2][NR];
    // bit 4 a + reg of em[sd][b]: child sd has the entry (r[b], cc[a][reg]) -- a row that lands on the row AND one that lands on the
    // column, inside the launch's columns and, on the diagonal tiles, r >= cc.  One register per (child, row), not one per entry
    unsigned em[2][NR];
};

template <int NA, int NR, bool DIAG>
__device__ __forceinline__ void gather_mono_prepare(const FrontDev& fd, int t, long long dp, int nf, int col_lo, int col_hi, const int (&r)[NR],
                                                    const int (&cc)[NA][4], GatherMono<NA, NR>& gm) {
    int outm[NA][4];                                               // -1: the column is outside the launch's [col_lo, col_hi)
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) outm[a][reg] = ((cc[a][reg] - col_lo) | (col_hi - 1 - cc[a][reg])) >> 31;
#pragma unroll
    for (int sd = 0; sd < 2; ++sd) {
        const int ch = fd.child[sd][t];
        const int chs = ch >= 0 ? ch : t;                          // no such child: every entry is absent, and Sc[0] is a safe address
        const int nochild = ch >> 31;
        const int npc = fd.npiv[chs], nbc = fd.nf[chs] - npc;
        gm.Sc[sd] = reinterpret_cast<const char*>(fd.S + fd.soff[chs]);
        const char* inv = reinterpret_cast<const char*>(fd.cinv[sd] + dp);        // uniform base, 32-bit byte offsets
        unsigned colbits = 0u;
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int y = *reinterpret_cast<const int*>(inv + 4u * (unsigned)min(cc[a][reg], nf - 1)) | nochild | outm[a][reg];   // -1: none
                colbits |= ((unsigned)~y >> 31) << (4 * a + reg);
                gm.colb[sd][a][reg] = __umul24(8u * (unsigned)nbc, (unsigned)(max(y, npc) - npc));
            }
#pragma unroll
        for (int b = 0; b < NR; ++b) {
            const int x = *reinterpret_cast<const int*>(inv + 4u * (unsigned)min(r[b], nf - 1)) | nochild | ((nf - 1 - r[b]) >> 31);   // -1: none
            gm.em[sd][b] = colbits & (unsigned)~(x >> 31);
            gm.rowb[sd][b] = 8u * (unsigned)(max(x, npc) - npc);
        }
    }
    if (DIAG) {
#pragma unroll
        for (int b = 0; b < NR; ++b) {
            unsigned tri = 0u;                                     // bit 4 a + reg: r[b] >= cc[a][reg]
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) tri |= ((unsigned)(cc[a][reg] - 1 - r[b]) >> 31) << (4 * a + reg);
            gm.em[0][b] &= tri; gm.em[1][b] &= tri;
        }
    }
}

// block row a: out[b][reg] = g0 + g1
template <int NA, int NR>
__device__ __forceinline__ void gather_mono_fetch(const GatherMono<NA, NR>& gm, int a, double (&out)[NR][4]) {
    double g[2][NR][4];
#pragma unroll
    for (int sd = 0; sd < 2; ++sd)
#pragma unroll
        for (int b = 0; b < NR; ++b)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) g[sd][b][reg] = *reinterpret_cast<const double*>(gm.Sc[sd] + (gm.colb[sd][a][reg] + gm.rowb[sd][b]));
#pragma unroll
    for (int b = 0; b < NR; ++b)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            double gs[2];
#pragma unroll
            for (int sd = 0; sd < 2; ++sd) {
                const int m = (int)(gm.em[sd][b] << (31 - (4 * a + reg))) >> 31;                 // all ones: the entry exists
                gs[sd] = __hiloint2double(__double2hiint(g[sd][b][reg]) & m, __double2loint(g[sd][b][reg]) & m);
            }
            out[b][reg] = gs[0] + gs[1];
        }
}

// Any other front: the child rows of a pair in either order, min / max per entry.
template <int NA, int NR>
__device__ __forceinline__ void gather_tile_any(const FrontDev& fd, int t, long long dp, int nf, const int (&r)[NR], const int (&cc)[NA][4],
                                                const bool (&ccok)[NA][4], double (&cv)[NA][NR][4]) {
    int rr[2][NR], cr[2][NA][4];
    const double* Sc[2];
    int npc[2], nbc[2];
#pragma unroll
    for (int sd = 0; sd < 2; ++sd) {
        const int ch = fd.child[sd][t];
        const int chs = ch >= 0 ? ch : t;
        npc[sd] = fd.npiv[chs]; nbc[sd] = fd.nf[chs] - npc[sd];
        Sc[sd] = fd.S + fd.soff[chs];
#pragma unroll
        for (int b = 0; b < NR; ++b) {
            rr[sd][b] = fd.cinv[sd][dp + min(r[b], nf - 1)];
            if (ch < 0 || r[b] >= nf) rr[sd][b] = -1;
        }
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                cr[sd][a][reg] = fd.cinv[sd][dp + min(cc[a][reg], nf - 1)];
                if (ch < 0 || !ccok[a][reg]) cr[sd][a][reg] = -1;
            }
    }
    double g0[NA][NR][4], g1[NA][NR][4];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NR; ++b)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const bool tri = r[b] >= cc[a][reg];
                {
                    const int x = rr[0][b], y = cr[0][a][reg];
                    const bool ok = tri && x >= 0 && y >= 0;
                    const int lo = min(x, y) - npc[0], hi = max(x, y) - npc[0];
                    g0[a][b][reg] = Sc[0][ok ? hi + (size_t)nbc[0] * lo : 0];
                    if (!ok) g0[a][b][reg] = 0.0;
                }
                {
                    const int x = rr[1][b], y = cr[1][a][reg];
                    const bool ok = tri && x >= 0 && y >= 0;
                    const int lo = min(x, y) - npc[1], hi = max(x, y) - npc[1];
                    g1[a][b][reg] = Sc[1][ok ? hi + (size_t)nbc[1] * lo : 0];
                    if (!ok) g1[a][b][reg] = 0.0;
                }
            }
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NR; ++b)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) cv[a][b][reg] = g0[a][b][reg] + g1[a][b][reg];
}

// GATHER (levels above the leaves, the launch that touches its columns first): the tile of C does not exist yet -- it is
// the sum of the children's Schur-complement entries that land there (the extend-add of these columns, left out of
// k_extend_gather), gathered here and written once.  `mask`: strong-BC pivots get their unit diagonal, as in the extend-add.
template <bool GATHER>
__global__ void __launch_bounds__(256, 4)      // 128 registers: four waves per SIMD (measured: -6 % against three)
k_trailing_mfma(FrontDev fd, const int* __restrict__ level_nodes, int first, int C0, int schur, int K0, int KW,
                const unsigned char* __restrict__ mask) {
    // Which (front, tile) this workgroup takes.  Workgroups are dealt round-robin over the 8 XCDs (each with its own L2) in
    // launch order, x fastest; the two or three tiles of a small front read the same rows of its factor panel.  On levels
    // of many fronts (a multiple of 8, at least 256) XCD x therefore takes the fronts x, x + 8, ... whole, tile after tile:
    // the panel leaves HBM once instead of once per tile (leaves 604 -> 552 us, levels 1-5 -2..-5 %).  The map is a
    // bijection of the grid whatever the placement really is.  Levels of fewer, larger fronts keep the launch order: their
    // tiles must spread over all eight XCDs (64 fronts: +8 % with the map; 8 unequal fronts: +75 %).
    int bxv = blockIdx.x, zv = blockIdx.z;
    {
        const int G = gridDim.x, n = gridDim.z;
        if (n >= 256 && (n & 7) == 0) {
            const int flat = bxv + G * zv, x = flat & 7, q = flat >> 3;
            zv = (q / G) * 8 + x; bxv = q % G;
        }
    }
    const int t = level_nodes[first + zv];
    const int np = fd.npiv[t];
    const int nf = fd.nf[t];
    const TrailRange tr = trail_range(schur, C0, K0, KW, np, nf);
    const int kc0 = tr.kc0, kw = tr.kw, col_lo = tr.col_lo, col_hi = tr.col_hi;
    if (kw <= 0) return;
    // tile from the linear block index: consecutive workgroups go to different XCDs, so a (row tile, column tile)
    // grid whose x extent is a multiple of 8 would pin every row-tile offset to one XCD -- and the lower triangle has
    // 8x more tiles at offset 0 than at offset 7.  The linear order spreads them evenly (measured: up to 2.2x).
    int bx, by;
    if (schur == 0 || schur == 3) {
        by = bxv & 1; bx = bxv >> 1;                               // two column tiles per panel
    } else {
        const int lin = bxv;
        int ti = (int)((sqrt(8.0 * lin + 1.0) - 1.0) * 0.5);
        while ((ti + 1) * (ti + 2) / 2 <= lin) ++ti;
        while (ti * (ti + 1) / 2 > lin) --ti;
        by = lin - ti * (ti + 1) / 2; bx = ti - by;                 // column tile by, row tile by + bx
    }
    // tiles are anchored at an even column: with the even leading dimension of the panel store every pair of rows
    // (2 rp, 2 rp + 1) of a tile is then one aligned 16-byte load
    const int cj = (col_lo & ~1) + by * TS;
    if (cj >= col_hi) return;
    const int ri = cj + bx * TS;                   // row tiles start at the column tile (lower triangle)
    if (ri >= nf) return;
    const FrontView fv = front_view(fd, t);
    // 16 factor columns per stage, two LDS buffers (20 KB each): the next stage travels global -> registers while the
    // matrix cores work on the current one, and one barrier per stage suffices
    constexpr int KC = 16;
    __shared__ __attribute__((aligned(16))) double si[2][KC][LSTR];   // rows of the tile:    si[.][k][r] = L[ri + r][kc0 + k0 + k]
    __shared__ __attribute__((aligned(16))) double sj[2][KC][LSTR];   // columns of the tile: sj[.][k][c] = L[cj + c][kc0 + k0 + k]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wr = (wv & 1) * 32, wc = (wv >> 1) * 32;     // this wave's quarter: rows wr.., columns wc..
    const int l15 = lane & 15, l4 = lane >> 4;
    // Staging with as little vector arithmetic as possible -- the vector ALU shares its issue slots with the matrix
    // cores, and address / mask arithmetic per load costs this kernel a fifth of its rate (micro-benchmark: 49 -> 60
    // TFLOP/s at K = 512, 32 -> 41 at K = 128).  The stage pointer is uniform; a thread keeps four constant 32-bit byte
    // offsets (rows 2 rp, 2 rp + 1 of the tile's row and column blocks, factor columns cg and cg + 8).  Rows past the
    // front are clamped to its last row pair (their products are never stored); only the last, partial stage is masked.
    const int rp = tid & 31, cg = tid >> 5;
    const int ldp = ldp_of(nf);
    const int rowi = min(ri + 2 * rp, ldp - 2), rowj = min(cj + 2 * rp, ldp - 2);
    const unsigned obi0 = 8u * (unsigned)(rowi + ldp * cg), obi1 = 8u * (unsigned)(rowi + ldp * (cg + 8));
    const unsigned obj0 = 8u * (unsigned)(rowj + ldp * cg), obj1 = 8u * (unsigned)(rowj + ldp * (cg + 8));
    const char* base = reinterpret_cast<const char*>(fv.P + (size_t)ldp * kc0);      // the K panel: always pivot columns
    const size_t stage_bytes = (size_t)ldp * KC * 8;
    d2 pi[2], pj[2];
    auto fetch = [&](const char* b) {
        pi[0] = *reinterpret_cast<const d2*>(b + obi0); pi[1] = *reinterpret_cast<const d2*>(b + obi1);
        pj[0] = *reinterpret_cast<const d2*>(b + obj0); pj[1] = *reinterpret_cast<const d2*>(b + obj1);
    };
    auto fetch_tail = [&](const char* b, int left) {       // left = factor columns this stage still has (1..15)
        const d2 z = {0.0, 0.0};
        const unsigned a0 = 8u * (unsigned)(ldp * min(cg, left - 1)), a1 = 8u * (unsigned)(ldp * min(cg + 8, left - 1));
        const d2 vi0 = *reinterpret_cast<const d2*>(b + 8u * (unsigned)rowi + a0), vi1 = *reinterpret_cast<const d2*>(b + 8u * (unsigned)rowi + a1);
        const d2 vj0 = *reinterpret_cast<const d2*>(b + 8u * (unsigned)rowj + a0), vj1 = *reinterpret_cast<const d2*>(b + 8u * (unsigned)rowj + a1);
        pi[0] = cg < left ? vi0 : z; pi[1] = cg + 8 < left ? vi1 : z;
        pj[0] = cg < left ? vj0 : z; pj[1] = cg + 8 < left ? vj1 : z;
    };
    if (kw >= KC) fetch(base); else fetch_tail(base, kw);
    base += stage_bytes;
    mfma_d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (mfma_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        *reinterpret_cast<d2*>(&si[0][cg + 8 * q][2 * rp]) = pi[q];
        *reinterpret_cast<d2*>(&sj[0][cg + 8 * q][2 * rp]) = pj[q];
    }
    __syncthreads();
    int cur = 0;
    // a tile on the diagonal of the front (row tile == column tile): the wave whose quarter lies entirely ABOVE the diagonal (rows 0..31,
    // columns 32..63) has nothing to store -- it only helps with the staging.  On the levels of small fronts a third to a half of the
    // tiles are diagonal ones (a Schur block of 174 rows: 3 of 6), so this is 8-12 % of their MFMA work, which is what those levels
    // spend about half of their time on (the tile-quantised work is ~2.5 x the algorithmic flops there).
    const bool idle_quarter = ri == cj && wr + 31 < wc;
    for (int k0 = 0; k0 < kw; k0 += KC) {
        const int left = kw - k0 - KC;             // factor columns behind this stage
        if (left > 0) {
            if (left >= KC) fetch(base); else fetch_tail(base, left);
            base += stage_bytes;
        }
        if (!idle_quarter) {
#pragma unroll
        for (int kk = 0; kk < KC; kk += 4) {
            // A: tile columns (index i), B: tile rows (index j); k = kk + (lane >> 4)
            const double a0 = sj[cur][kk + l4][wc + l15], a1 = sj[cur][kk + l4][wc + 16 + l15];
            const double b0 = si[cur][kk + l4][wr + l15], b1 = si[cur][kk + l4][wr + 16 + l15];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        }
        if (left > 0) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                *reinterpret_cast<d2*>(&si[cur ^ 1][cg + 8 * q][2 * rp]) = pi[q];
                *reinterpret_cast<d2*>(&sj[cur ^ 1][cg + 8 * q][2 * rp]) = pj[q];
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    if (idle_quarter) return;                      // (behind the last barrier of the K loop: nothing of this quarter is stored)
    // C -= D with all of the tile's loads in flight at once (entries outside the tile's part of the lower triangle load
    // from a safe address and are not stored).  D[i][j]: i = l4 + 4*reg -> tile column, j = l15 -> tile row
    bool cok[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int cc = cj + wc + 16 * a + l4 + 4 * reg;
            cok[a][reg] = cc >= col_lo && cc < col_hi;
        }
    auto col_ptr = [&](int a, int reg) {                       // safe: [r] below stays inside the panel store
        const int cc = cj + wc + 16 * a + l4 + 4 * reg;
        return cok[a][reg] ? fv.col(cc) : fv.P - (nf - 1);
    };
    // Where the launch's columns live: all in the Schur arena (col_lo >= np: the Schur updates of the left-looking levels, entry
    // (r, c) at S + (r - np) + (nf - np) (c - np)), all in the panel store (col_hi <= np: P + r + ldp c), or both (-1: col_ptr per
    // entry).  The one-store cases keep byte offsets in 32 bits, guarded by the size of the block.
    const int st_side = (col_lo >= np && nf - np <= (1 << 14)) ? 1 : (col_hi <= np && (size_t)ldp * (size_t)np < (size_t)(1u << 28)) ? 0 : -1;
    const int st_ld = st_side == 1 ? nf - np : ldp, st_c0 = st_side == 1 ? np : 0;
    char* const st_base = reinterpret_cast<char*>(st_side == 1 ? fv.S : fv.P);
    // block row a of the wave's quarter: strong-BC pivots get their unit diagonal (gathering launches), C = cva - D is stored
    auto finish = [&](int a, const double (&cva)[2][4]) {
        double x[2][4];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) x[b][reg] = cva[b][reg];
        if (GATHER && mask && bx == 0) {                       // diagonal entries exist only in the tiles on the diagonal (a uniform branch)
            const int* gd = fd.dofs + fd.doff[t];
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int cc = cj + wc + 16 * a + l4 + 4 * reg;
                    const int r = ri + wr + 16 * b + l15;
                    if (r == cc && cok[a][reg] && cc < np && mask[gd[r]]) x[b][reg] = 1.0;
                }
        }
        if (st_side >= 0) {
            // all of the launch's columns in one store: a uniform base and 32-bit byte offsets, a column term plus a row term
            unsigned co[4], ro[2];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) co[reg] = 8u * (unsigned)st_ld * (unsigned)(cj + wc + 16 * a + l4 + 4 * reg - st_c0);
#pragma unroll
            for (int b = 0; b < 2; ++b) ro[b] = 8u * (unsigned)(ri + wr + 16 * b + l15 - st_c0);
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int cc = cj + wc + 16 * a + l4 + 4 * reg;
                    const int r = ri + wr + 16 * b + l15;
                    if (cok[a][reg] && r < nf && r >= cc) *reinterpret_cast<double*>(st_base + (co[reg] + ro[b])) = x[b][reg] - acc[a][b][reg];
                }
            return;
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int cc = cj + wc + 16 * a + l4 + 4 * reg;
                const int r = ri + wr + 16 * b + l15;
                if (cok[a][reg] && r < nf && r >= cc) col_ptr(a, reg)[r] = x[b][reg] - acc[a][b][reg];
            }
    };
    int gr[2], gc[2][4];
#pragma unroll
    for (int b = 0; b < 2; ++b) gr[b] = ri + wr + 16 * b + l15;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) gc[a][reg] = cj + wc + 16 * a + l4 + 4 * reg;
    if (GATHER && fd.cmono[t] == 3) {
        // both children land in increasing rows: per-column addressing, one block row at a time (gather_mono_*)
        GatherMono<2, 2> gm;
        if (bx == 0) gather_mono_prepare<2, 2, true>(fd, t, fd.doff[t], nf, col_lo, col_hi, gr, gc, gm);
        else gather_mono_prepare<2, 2, false>(fd, t, fd.doff[t], nf, col_lo, col_hi, gr, gc, gm);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            double cva[2][4];
            gather_mono_fetch<2, 2>(gm, a, cva);
            finish(a, cva);
        }
        return;
    }
    double cv[2][2][4];
    if (!GATHER) {
        double* cp[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) cp[a][reg] = col_ptr(a, reg);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int cc = cj + wc + 16 * a + l4 + 4 * reg;
                    const int r = ri + wr + 16 * b + l15;
                    const bool ok = cok[a][reg] && r < nf && r >= cc;
                    cv[a][b][reg] = cp[a][reg][ok ? r : nf - 1];
                }
    } else gather_tile_any<2, 2>(fd, t, fd.doff[t], nf, gr, gc, cok, cv);      // the sum of the two children's entries that land on this lane's two rows and eight columns
#pragma unroll
    for (int a = 0; a < 2; ++a) finish(a, cv[a]);
}

// ---- the narrow (schur 0) update cut finer, for launches that do not fill the chip.  At the top of the tree a narrow update is a
// few dozen 64 x 64 tiles whose waves each walk K MFMAs behind K / 16 staged loads: the launch lasts as long as that one chain
// (12 us at K = 128, 30 at K = 512, whatever the number of tiles).  Here a workgroup takes a 32 x 32 tile and a wave ONE 16 x 16
// block: K / 4 MFMAs, a quarter of the chain, four times the workgroups.  No LDS: both MFMA operands are 16 consecutive rows of a
// factor column per k (one 128-byte segment), loaded straight to registers in batches of 32 factor columns (two batches, 32 loads,
// in flight per lane), the next batch requested before the products of the current one.  K range, column range and the gathering epilogue
// are those of k_trailing_mfma with schur == 0; the host takes this kernel when the K range is a multiple of 64.
template <bool GATHER>
__global__ void __launch_bounds__(256, 2)
k_trailing_fine(FrontDev fd, const int* __restrict__ level_nodes, int first, int C0, int K0, const unsigned char* __restrict__ mask) {
    const int t = level_nodes[first + blockIdx.z];
    const int np = fd.npiv[t];
    const int nf = fd.nf[t];
    const TrailRange tr = trail_range(0, C0, K0, NBO, np, nf);
    const int kc0 = tr.kc0, kw = tr.kw, col_lo = tr.col_lo, col_hi = tr.col_hi;
    if (kw <= 0) return;
    constexpr int FT = 32;                                       // tile edge
    const int bxv = (int)blockIdx.x;
    const int by = bxv & 3, bx = bxv >> 2;                       // four column tiles per panel
    const int cj = (col_lo & ~1) + by * FT;
    if (cj >= col_hi) return;
    const int ri = cj + bx * FT;                                 // row tiles start at the column tile (lower triangle)
    if (ri >= nf) return;
    const FrontView fv = front_view(fd, t);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wr = (wv & 1) * 16, wc = (wv >> 1) * 16;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int ldp = ldp_of(nf);
    // operand rows: A = tile columns (D index i), B = tile rows (D index j); rows past the front are clamped (never stored)
    const double* pa = fv.P + min(cj + wc + l15, nf - 1) + (size_t)ldp * (kc0 + l4);
    const double* pb = fv.P + min(ri + wr + l15, nf - 1) + (size_t)ldp * (kc0 + l4);
    const size_t kstep = (size_t)ldp * 4;
    constexpr int KB = 32, NS = KB / 4;                          // factor columns per batch, k-steps per batch (two batches in flight)
    double a0[NS], b0[NS], a1[NS], b1[NS];
    mfma_d4 acc = (mfma_d4){0.0, 0.0, 0.0, 0.0};
    const int nbatch = kw / KB;                                  // the host guarantees kw % KB == 0
#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_) { a0[s_] = pa[kstep * s_]; b0[s_] = pb[kstep * s_]; }
    for (int bt = 0; bt < nbatch; bt += 2) {
        const bool more1 = bt + 1 < nbatch, more2 = bt + 2 < nbatch;
        if (more1) {
#pragma unroll
            for (int s_ = 0; s_ < NS; ++s_) { a1[s_] = pa[kstep * (NS * (bt + 1) + s_)]; b1[s_] = pb[kstep * (NS * (bt + 1) + s_)]; }
        }
#pragma unroll
        for (int s_ = 0; s_ < NS; ++s_) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[s_], b0[s_], acc, 0, 0, 0);
        if (more2) {
#pragma unroll
            for (int s_ = 0; s_ < NS; ++s_) { a0[s_] = pa[kstep * (NS * (bt + 2) + s_)]; b0[s_] = pb[kstep * (NS * (bt + 2) + s_)]; }
        }
        if (more1) {
#pragma unroll
            for (int s_ = 0; s_ < NS; ++s_) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[s_], b1[s_], acc, 0, 0, 0);
        }
    }
    // epilogue: D[i = l4 + 4 reg -> column][j = l15 -> row]
    const int r = ri + wr + l15;
    bool cok[4];
    double* cp[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int cc = cj + wc + l4 + 4 * reg;
        cok[reg] = cc >= col_lo && cc < col_hi && r < nf && r >= cc;
        cp[reg] = cok[reg] ? fv.col(cc) + r : fv.P;              // safe address for the lanes that store nothing
    }
    double cv[4];
    if (!GATHER) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) cv[reg] = *cp[reg];
    } else {
        const long long dp = fd.doff[t];
        int gr[1] = {r}, gc[1][4];
        bool ccok[1][4];
        double g[1][1][4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            gc[0][reg] = cj + wc + l4 + 4 * reg;
            ccok[0][reg] = gc[0][reg] >= col_lo && gc[0][reg] < col_hi;
        }
        if (fd.cmono[t] == 3) {                                  // both children land in increasing rows: per-column addressing
            GatherMono<1, 1> gm;
            if (bx == 0) gather_mono_prepare<1, 1, true>(fd, t, dp, nf, col_lo, col_hi, gr, gc, gm);
            else gather_mono_prepare<1, 1, false>(fd, t, dp, nf, col_lo, col_hi, gr, gc, gm);
            gather_mono_fetch<1, 1>(gm, 0, g[0]);
        } else gather_tile_any<1, 1>(fd, t, dp, nf, gr, gc, ccok, g);
        const int* gd = fd.dofs + dp;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int cc = cj + wc + l4 + 4 * reg;
            cv[reg] = g[0][0][reg];
            if (mask && r == cc && cok[reg] && cc < np && mask[gd[r]]) cv[reg] = 1.0;
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
        if (cok[reg]) *cp[reg] = cv[reg] - acc[reg];
}

// ------------------------------------------------------------------------------------------ solves
// M^-1 = L^-T L^-1 applied level by level.  Each sweep is split per level into a sequential part on
// the triangular pivot block L11 (one workgroup per front, panels chained through the stored diagonal
// block inverses) and a wide part on the rectangular block L21 (plain / transposed GEMV spread over
// many workgroups), which holds most of the factor's bytes.

// ---- small fronts (tree levels whose largest pivot block is <= WIDE_NP): one workgroup per front does the
// whole sweep of that front; inner loops are unrolled so that many loads are in flight per thread.

// Both kernels are latency-bound per workgroup (a front is 100-300 KB, a level has one to a few rounds of workgroups):
// every phase spreads its loads over all 256 threads -- lanes along the rows of the column-major factor, thread groups
// along the columns, partial sums joined through LDS -- so that a phase is one or two batches of loads in flight, not a
// loop of dependent batches on 32 or 100 active threads (measured at 1M DOF: levels 1-3 70-89 -> see DESIGN.md).
constexpr int SMALL_PART = 512;      // doubles of LDS for the partial sums of a phase

// forward: y_p = L11^-1 v_p -> yv ; v_B -= L21 y_p
__global__ void __launch_bounds__(256, 4)
k_front_fwd_small(FrontDev fd, const int* __restrict__ level_nodes, double* __restrict__ v, double* __restrict__ yv) {
    const int t = level_nodes[blockIdx.x];
    const int np = fd.npiv[t], nf = fd.nf[t];
    if (np == 0) return;
    const double* F = fd.P + fd.poff[t];                       // the factor columns [L11; L21]
    const int ldp = ldp_of(nf);
    const int* gd = fd.dofs + fd.doff[t];
    extern __shared__ double sh[];
    double* y = sh;              // np
    double* part = sh + np;      // SMALL_PART
    const int tid = threadIdx.x;
    for (int p = tid; p < np; p += 256) y[p] = v[gd[p]];
    __syncthreads();
    const int npan = (np + NB - 1) / NB;
    for (int k = 0; k < npan; ++k) {
        const int c0 = k * NB, wb = min(NB, np - c0);
        const double* Li = fd.Linv + fd.linvoff[t] + (size_t)k * NB * NB;
        {   // y_k = Linv_k y[c0 .. c0 + wb): thread (row r, group g) takes the columns g, g + 8, g + 16, g + 24 that are <= r
            const int r = tid & 31, g = tid >> 5;
            double a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int mm = g + 8 * q; a[q] = (mm <= r && r < wb) ? Li[r + NB * mm] : 0.0; }
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int mm = g + 8 * q; s += a[q] * y[c0 + min(mm, wb - 1)]; }
            part[32 * g + r] = s;
        }
        __syncthreads();
        if (tid < 32) {
            double s = 0.0;
#pragma unroll
            for (int g = 0; g < 8; ++g) s += part[32 * g + tid];
            part[256 + tid] = s;                               // y_k, read by the update below
            if (tid < wb) y[c0 + tid] = s;
        }
        __syncthreads();
        // the pivot rows below the panel: y[r] -= L11[r][c0 .. c0 + wb) y_k; thread (row slot tid & 127, half tid >> 7)
        const int r1 = c0 + wb;
        if (r1 < np) {
            const int h = tid >> 7;
            for (int rb = r1; rb < np; rb += 128) {
                const int r = rb + (tid & 127);
                double a[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) { const int mm = 16 * h + q; a[q] = (r < np && mm < wb) ? F[r + (size_t)ldp * (c0 + mm)] : 0.0; }
                double s = 0.0;
#pragma unroll
                for (int q = 0; q < 16; ++q) s += a[q] * part[256 + 16 * h + q];
                if (h) part[tid & 127] = s;
                __syncthreads();
                if (!h && r < np) y[r] -= s + part[tid & 127];
                __syncthreads();
            }
        }
    }
    for (int p = tid; p < np; p += 256) yv[gd[p]] = y[p];
    // v_B -= L21 y: row slots of 64, 128 or 256 and 4, 2 or 1 column groups, 16 loads in flight per thread
    const int nb = nf - np;
    if (nb > 0) {
        const int slots = nb <= 64 ? 64 : nb <= 128 ? 128 : 256, G = 256 / slots;
        const int rs = tid % slots, g = tid / slots;
        const int cper = (np + G - 1) / G, cbeg = g * cper, cend = min(np, cbeg + cper);
        for (int rb = 0; rb < nb; rb += slots) {
            const int r = rb + rs;
            const double* row = F + np + min(r, nb - 1);
            double s = 0.0;
            // 32 loads in flight per thread: on the levels that fit the chip in one round of workgroups the sweep lasts as long as one
            // workgroup's chain of dependent load rounds does
            for (int cb = cbeg; cb < cend; cb += 32) {
                double a[32];
#pragma unroll
                for (int q = 0; q < 32; ++q) a[q] = cb + q < cend ? row[(size_t)ldp * (cb + q)] : 0.0;
#pragma unroll
                for (int q = 0; q < 32; ++q) s += a[q] * y[min(cb + q, np - 1)];
            }
            if (G > 1) {
                if (g) part[slots * (g - 1) + rs] = s;
                __syncthreads();
                if (!g)
                    for (int gg = 1; gg < G; ++gg) s += part[slots * (gg - 1) + rs];
            }
            if (!g && r < nb) atomicAdd(&v[gd[np + r]], -s);
            if (G > 1) __syncthreads();
        }
    }
}

// backward: x_p = L11^-T (y_p - L21^T x_B)
template <bool BFLY>
__global__ void __launch_bounds__(256, 4)
k_front_bwd_small(FrontDev fd, const int* __restrict__ level_nodes, const double* __restrict__ sv, double* __restrict__ xv) {
    const int t = level_nodes[blockIdx.x];
    const int np = fd.npiv[t], nf = fd.nf[t];
    if (np == 0) return;
    const double* F = fd.P + fd.poff[t];                       // the factor columns [L11; L21]
    const int ldp = ldp_of(nf);
    const int* gd = fd.dofs + fd.doff[t];
    extern __shared__ double sh[];
    double* x = sh;              // nf: s_p (then x_p) in [0, np), x_B behind
    double* part = sh + nf;      // SMALL_PART
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int p = tid; p < nf; p += 256) x[p] = p < np ? sv[gd[p]] : xv[gd[p]];
    __syncthreads();
    // s_p -= L21^T x_B: a wave takes eight columns at a time, lanes along the rows, up to four row chunks: 32 loads in
    // flight per lane, then eight wave reductions
    const int nb = nf - np;
    if (nb > 0) {
        for (int cb = 8 * wid; cb < np; cb += 32) {
            double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int rb = 0; rb < nb; rb += 256) {
                double a[8][4];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const double* col = F + np + (size_t)ldp * min(cb + q, np - 1);
#pragma unroll
                    for (int u = 0; u < 4; ++u) { const int r = rb + lane + 64 * u; a[q][u] = r < nb ? col[r] : 0.0; }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int r = rb + lane + 64 * u;
                    const double xr = x[np + min(r, nb - 1)];
#pragma unroll
                    for (int q = 0; q < 8; ++q) s[q] += a[q][u] * xr;
                }
            }
            if (BFLY) {
                int q;
                const double tot = wave_sum_cols<8>(s, lane, q);
                if (!(lane & 7) && cb + q < np) x[cb + q] -= tot;            // a column belongs to one wave
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const double tot = wave_sum(s[q]);
                    if (lane == 0 && cb + q < np) x[cb + q] -= tot;
                }
            }
        }
        __syncthreads();
    }
    const int npan = (np + NB - 1) / NB;
    for (int k = npan - 1; k >= 0; --k) {
        const int c0 = k * NB, wb = min(NB, np - c0);
        const double* Li = fd.Linv + fd.linvoff[t] + (size_t)k * NB * NB;
        // s_k -= L11[r1 .., panel]^T x[r1 ..): the pivot rows below the panel (solved already); wave = eight columns
        const int r1 = c0 + wb, nr = np - r1;
        if (nr > 0) {
            const int cb = 8 * wid;
            double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int rb = 0; rb < nr; rb += 256) {
                double a[8][4];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const double* col = F + r1 + (size_t)ldp * (c0 + min(cb + q, wb - 1));
#pragma unroll
                    for (int u = 0; u < 4; ++u) { const int r = rb + lane + 64 * u; a[q][u] = r < nr ? col[r] : 0.0; }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int r = rb + lane + 64 * u;
                    const double xr = x[r1 + min(r, nr - 1)];
#pragma unroll
                    for (int q = 0; q < 8; ++q) s[q] += a[q][u] * xr;
                }
            }
            if (BFLY) {
                int q;
                const double tot = wave_sum_cols<8>(s, lane, q);
                if (!(lane & 7) && cb + q < wb) x[c0 + cb + q] -= tot;
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const double tot = wave_sum(s[q]);
                    if (lane == 0 && cb + q < wb) x[c0 + cb + q] -= tot;
                }
            }
            __syncthreads();
        }
        {   // x_k = Linv_k^T s_k: thread (column c, group g) takes the rows c + g, c + g + 8, ... < wb
            const int c = tid & 31, g = tid >> 5;
            double a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int r = c + g + 8 * q; a[q] = (r < wb && c < wb) ? Li[r + NB * c] : 0.0; }
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int r = c + g + 8 * q; s += a[q] * x[c0 + min(r, wb - 1)]; }
            part[32 * g + c] = s;
        }
        __syncthreads();
        if (tid < wb) {
            double s = 0.0;
#pragma unroll
            for (int g = 0; g < 8; ++g) s += part[32 * g + tid];
            x[c0 + tid] = s;
        }
        __syncthreads();
    }
    for (int p = tid; p < np; p += 256) xv[gd[p]] = x[p];
}

// ---- wide levels (few fronts, or large pivot blocks): the sweeps are four plain matrix-vector products per level
//
//   forward    y_p = X b_p                 (k_sweep_gemv_n<true>)     v_B -= L21 y_p          (k_sweep_gemv_n<false>)
//   backward   s_p = y_p - L21^T x_B       (k_sweep_gemv_t<false>)    x_p  = X^T s_p          (k_sweep_gemv_t<true>)
//
// with X = L11^-1 formed explicitly after the factorisation (k_xinv below).  Substitution through L11 is a chain of one
// dependent step per 128 pivot columns -- at the top of the tree (pivot blocks of 1000-1500 columns, a handful of
// fronts) that chain was 10-12 launches of ~9 us per sweep and level with the chip idle; as products with X and L21
// every sweep is two launches per level whose 128 x 128 tiles spread over the whole chip, and each factor byte is
// still read exactly once.  Partial sums of a tile are added atomically (the output entries are zeroed by one memset
// per sweep).

// 128 x 128 tile, 256 threads: thread (row lr, column half ch) keeps 32 loads in flight at a time
template <bool TRI>
__device__ __forceinline__ void gemv_n_tile(const FrontDev& fd, int t, int bx, const double* __restrict__ in, double* __restrict__ out) {
    const int np = fd.npiv[t], nf = fd.nf[t];
    if (np == 0) return;
    const int nct = (np + 127) / 128;
    int ti, tj;                                              // row tile, column tile
    if (TRI) {
        const int lin = bx;
        if (lin >= nct * (nct + 1) / 2) return;
        ti = (int)((sqrt(8.0 * lin + 1.0) - 1.0) * 0.5);
        while ((ti + 1) * (ti + 2) / 2 <= lin) ++ti;
        while (ti * (ti + 1) / 2 > lin) --ti;
        tj = lin - ti * (ti + 1) / 2;
    } else {
        const int nrt = (nf - np + 127) / 128;
        if (bx >= nrt * nct) return;
        ti = bx / nct; tj = bx % nct;
    }
    const int* gd = fd.dofs + fd.doff[t];
    const int ld = TRI ? ldx_of(np) : ldp_of(nf);
    const double* M = TRI ? fd.X + fd.xoff[t] : fd.P + fd.poff[t] + np;       // L21 starts at row np of the pivot columns
    const int nrows = TRI ? np : nf - np;
    // L21: the pivot columns are dealt evenly over the front's column tiles (np = 210: 106 + 104 columns, not 128 + 82 -- a
    // workgroup lasts as long as its longest thread); X keeps square tiles, its triangle is enumerated that way
    const int cw = TRI ? 128 : ((np + nct - 1) / nct + 1) & ~1, hw = cw / 2;
    const int r0 = 128 * ti, c0 = cw * tj;
    __shared__ double xs[128];
    __shared__ double part[128];
    const int tid = threadIdx.x, lr = tid & 127, ch = tid >> 7;
    if (tid < 128) xs[tid] = (tid < cw && c0 + tid < np) ? in[gd[c0 + tid]] : 0.0;
    const int r = r0 + lr;
    const double* row = M + r + (size_t)ld * (c0 + hw * ch);
    // triangular tiles on the diagonal: only columns <= row
    const int cmax = min(np - c0 - hw * ch, hw);             // columns of this half inside the pivot block
    const int clim = (TRI && ti == tj) ? min(cmax, lr - hw * ch + 1) : cmax;
    double a[32];
    double s = 0.0;
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int k = 0; k < 32; ++k) a[k] = (r < nrows && 32 * h + k < clim) ? row[(size_t)ld * (32 * h + k)] : 0.0;
#pragma unroll
        for (int k = 0; k < 32; ++k) s += a[k] * xs[hw * ch + 32 * h + k];              // hw <= 64: inside xs
    }
    if (ch) part[lr] = s;
    __syncthreads();
    if (!ch && r < nrows) {
        s += part[lr];
        if (TRI) atomicAdd(&out[gd[r]], s);
        else atomicAdd(&out[gd[np + r]], -s);
    }
}
template <bool TRI>
__global__ void __launch_bounds__(256)
k_sweep_gemv_n(FrontDev fd, const int* __restrict__ level_nodes, int first, const double* __restrict__ in, double* __restrict__ out) {
    gemv_n_tile<TRI>(fd, level_nodes[first + blockIdx.y], (int)blockIdx.x, in, out);
}

// transposed products: tile of 128 rows x 128 columns, wave w owns columns 32 w .. 32 w + 31 with its lanes along the
// (contiguous) rows, 64 loads in flight per lane; per column one wave reduction
template <bool TRI>
__device__ __forceinline__ void gemv_t_tile(const FrontDev& fd, int t, int bx, const double* __restrict__ in, double* __restrict__ out) {
    const int np = fd.npiv[t], nf = fd.nf[t];
    if (np == 0) return;
    const int nct = (np + 127) / 128;
    int ti, tj;
    if (TRI) {
        const int lin = bx;
        if (lin >= nct * (nct + 1) / 2) return;
        ti = (int)((sqrt(8.0 * lin + 1.0) - 1.0) * 0.5);
        while ((ti + 1) * (ti + 2) / 2 <= lin) ++ti;
        while (ti * (ti + 1) / 2 > lin) --ti;
        tj = lin - ti * (ti + 1) / 2;
    } else {
        const int nrt = (nf - np + 127) / 128;
        if (bx >= nrt * nct) return;
        ti = bx / nct; tj = bx % nct;
    }
    const int* gd = fd.dofs + fd.doff[t];
    const int ld = TRI ? ldx_of(np) : ldp_of(nf);
    const double* M = TRI ? fd.X + fd.xoff[t] : fd.P + fd.poff[t] + np;
    const int nrows = TRI ? np : nf - np;
    const int rbase = TRI ? 0 : np;                          // front row of M's row 0
    const int r0 = 128 * ti, c0 = 128 * tj;
    __shared__ double xs[128];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < 128) xs[tid] = (r0 + tid < nrows) ? in[gd[rbase + r0 + tid]] : 0.0;
    const int ra = r0 + lane, rb = r0 + lane + 64;
    double a0[32], a1[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const int c = c0 + 32 * wv + k;
        const double* col = M + (size_t)ld * c;
        // triangular: rows >= column
        const bool ca = c < np && ra < nrows && (!TRI || ra >= c);
        const bool cb = c < np && rb < nrows && (!TRI || rb >= c);
        a0[k] = ca ? col[ra] : 0.0;
        a1[k] = cb ? col[rb] : 0.0;
    }
    __syncthreads();
    const double x0 = xs[lane], x1 = xs[lane + 64];
    // the wave's 32 column sums in one butterfly (wave_sum_cols), out in ONE atomic instruction of 32 lanes
    double p[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) p[k] = a0[k] * x0 + a1[k] * x1;
    int col;
    const double sum = wave_sum_cols<32>(p, lane, col);
    const int c = c0 + 32 * wv + col;
    if (!(lane & 1) && c < np) atomicAdd(&out[gd[c]], TRI ? sum : -sum);
}
template <bool TRI>
__global__ void __launch_bounds__(256)
k_sweep_gemv_t(FrontDev fd, const int* __restrict__ level_nodes, int first, const double* __restrict__ in, double* __restrict__ out) {
    gemv_t_tile<TRI>(fd, level_nodes[first + blockIdx.y], (int)blockIdx.x, in, out);
}

// s_p = y_p - L21^T x_B with one workgroup per 16 pivot columns and ALL boundary rows of the front (no atomics, fixed
// summation order): the better shape for the many medium fronts of the middle levels, where a front's L21 is a few
// hundred rows; the tiled kernel above takes over where one workgroup per 32 columns could not pull the block out of HBM.
constexpr int BB_COLS = 16;
// ATOMIC: the sums are subtracted from sv with atomic adds (the W form of the sweeps, where other workgroups of the same launch add
// to the same entries)
template <bool BFLY, bool ATOMIC>
__device__ __forceinline__ void bnd_cols_block(const FrontDev& fd, int t, int bx, double* __restrict__ sv, const double* __restrict__ xv, double* xs) {
    const int np = fd.npiv[t], nf = fd.nf[t];
    const int nb = nf - np;
    const int c0 = bx * BB_COLS;
    if (c0 >= np || nb == 0) return;
    const int* gd = fd.dofs + fd.doff[t];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int r = tid; r < nb; r += 256) xs[r] = xv[gd[np + r]];
    __syncthreads();
    // a wave owns four columns; 4 columns x 8 row chunks = 32 loads in flight per lane (the upper levels have only one
    // or two workgroups per CU: what is in flight per wave is what pulls the block out of HBM)
    const int ldp = ldp_of(nf);
    const double* L21 = fd.P + fd.poff[t] + np;          // rows np.., column c at + ldp * c
    const int cb = c0 + 4 * wv;
    const double* col[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) col[k] = L21 + (size_t)ldp * min(cb + k, np - 1);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int rb = 0; rb < nb; rb += 512) {
        double a[4][8];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int r = rb + lane + 64 * u; a[k][u] = r < nb ? col[k][r] : 0.0; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double xr = xs[min(rb + lane + 64 * u, nb - 1)];
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] += a[k][u] * xr;
        }
    }
    if (BFLY) {
        int k;
        const double tot = wave_sum_cols<4>(s, lane, k);
        if (!(lane & 15) && cb + k < np) { if (ATOMIC) atomicAdd(&sv[gd[cb + k]], -tot); else sv[gd[cb + k]] -= tot; }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double tot = wave_sum(s[k]);
            if (lane == 0 && cb + k < np) { if (ATOMIC) atomicAdd(&sv[gd[cb + k]], -tot); else sv[gd[cb + k]] -= tot; }
        }
    }
}
template <bool BFLY>
__global__ void __launch_bounds__(256)
k_sweep_bnd_cols(FrontDev fd, const int* __restrict__ level_nodes, int first, double* __restrict__ sv, const double* __restrict__ xv) {
    extern __shared__ double xs_bnd[];                   // nb
    bnd_cols_block<BFLY, false>(fd, level_nodes[first + blockIdx.y], (int)blockIdx.x, sv, xv, xs_bnd);
}

// ---- the W form of the wide levels (option "sweep_w"): with W = L21 X stored in the place of L21 (k_w_inplace, beside the
// factorisation like X itself) both products of a level read the SAME input,
//   forward    y_p = X b_p,  v_B -= W b_p            backward   x_p = X^T y_p - W^T x_B,
// so a level is ONE launch per direction instead of two dependent ones: the product with X -- ~10 us whatever it moves, the chip
// mostly idle -- runs beside the tiles of W instead of in front of them.  The bytes are the same (W has the shape of L21).
__global__ void __launch_bounds__(256)
k_sweep_fwd_w(FrontDev fd, const int* __restrict__ level_nodes, int first, int nx, double* __restrict__ v, double* __restrict__ y) {
    const int t = level_nodes[first + blockIdx.y];
    if ((int)blockIdx.x < nx) gemv_n_tile<true>(fd, t, (int)blockIdx.x, v, y);
    else gemv_n_tile<false>(fd, t, (int)blockIdx.x - nx, v, v);          // reads the pivot entries of v, adds to the boundary entries
}
template <bool BFLY>
__global__ void __launch_bounds__(256)
k_sweep_bwd_w(FrontDev fd, const int* __restrict__ level_nodes, int first, int nx, const double* __restrict__ y, double* __restrict__ x) {
    extern __shared__ double xs_bnd[];                   // nb
    const int t = level_nodes[first + blockIdx.y];
    if ((int)blockIdx.x < nx) gemv_t_tile<true>(fd, t, (int)blockIdx.x, y, x);
    else bnd_cols_block<BFLY, true>(fd, t, (int)blockIdx.x - nx, x, x, xs_bnd);     // reads the boundary entries of x, adds to the pivot entries
}

// X = L11^-1 beyond its 128 x 128 diagonal blocks (which k_diag_block leaves in place), by recursive doubling: at block
// size bs = 128, 256, 512, ... the inverse of every aligned 2 bs block [[A, 0], [C, B]] of L11 is completed from the
// inverses XA, XB of its halves,  X_BA = -XB (C XA):
//   PHASE 0:  T = C XA  (into Xtmp, at the place of X_BA);   PHASE 1:  X_BA = -XB T.
// One workgroup per 128 x 64 tile of the result; fp64 MFMA with the product formed transposed (stores along rows).
// Entries above the diagonal of X are never read as data: triangular operands are masked while they are staged.
// Tile TM x TN per workgroup (four waves, 2 x 2): 128 x 64 where a level has many fronts, 64 x 32 at the top of the tree
// (a handful of fronts: more, shorter workgroups -- the K loop of one tile is the critical path there).
template <int PHASE, int TM, int TN>
__global__ void __launch_bounds__(256)
k_xinv(FrontDev fd, const int* __restrict__ level_nodes, int first, int bs) {
    const int t = level_nodes[first + blockIdx.y];
    const int np = fd.npiv[t];
    const int rts = bs / TM, cts = bs / TN;
    int lin = blockIdx.x;
    const int ct = lin % cts; lin /= cts;
    const int rt = lin % rts;
    const int pair = lin / rts;
    const int a0 = 2 * pair * bs, b0 = a0 + bs;
    if (b0 >= np) return;
    const int mB = min(bs, np - b0);
    const int r0 = rt * TM;
    if (r0 >= mB) return;
    const int c0 = ct * TN;
    const int nf = fd.nf[t], ldx = ldx_of(np);
    const double* F = fd.P + fd.poff[t];
    double* X = fd.X + fd.xoff[t];
    double* T = fd.Xtmp + fd.xoff[t];
    // XA is lower triangular: its rows k < c0 vanish in the columns >= c0;  XB likewise: columns k > row vanish
    const int k_lo = PHASE == 0 ? (c0 & ~15) : 0;
    const int k_hi = PHASE == 0 ? bs : min(mB, r0 + TM);
    constexpr int KC = 16, SA = TM + 16, SB = TN + 16;
    constexpr int GA = 256 / TM, QA = KC / GA;            // staging of A: row lr, k = kq + GA q
    constexpr int QB = TN / 16;                           // staging of B: k = kb, column cb + 16 q
    constexpr int MR = TM / 32, NC = TN / 32;             // 16 x 16 MFMA blocks per wave: rows, columns
    __shared__ double sA[2][KC][SA];                      // sA[.][k][r]: the operand whose rows are the result's rows
    __shared__ double sB[2][KC][SB];                      // sB[.][k][c]: the operand whose columns are the result's columns
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int lr = tid % TM, kq = tid / TM;
    const int kb = tid & 15, cb = tid >> 4;
    const bool rok = r0 + lr < mB;
    double pa[QA], pb[QB];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < QA; ++q) {
            const int k = k0 + kq + GA * q;
            if (PHASE == 0) pa[q] = (rok && k < k_hi) ? F[(b0 + r0 + lr) + (size_t)ldp_of(nf) * (a0 + k)] : 0.0;
            else pa[q] = (rok && k < k_hi && k <= r0 + lr) ? X[(b0 + r0 + lr) + (size_t)ldx * (b0 + k)] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < QB; ++q) {
            const int k = k0 + kb, c = c0 + cb + 16 * q;
            if (PHASE == 0) pb[q] = (k < k_hi && k >= c) ? X[(a0 + k) + (size_t)ldx * (a0 + c)] : 0.0;
            else pb[q] = (k < k_hi) ? T[(b0 + k) + (size_t)ldx * (a0 + c)] : 0.0;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int q = 0; q < QA; ++q) sA[buf][kq + GA * q][lr] = pa[q];
#pragma unroll
        for (int q = 0; q < QB; ++q) sB[buf][kb][cb + 16 * q] = pb[q];
    };
    mfma_d4 acc[NC][MR];
#pragma unroll
    for (int jc = 0; jc < NC; ++jc)
#pragma unroll
        for (int ir = 0; ir < MR; ++ir) acc[jc][ir] = (mfma_d4){0.0, 0.0, 0.0, 0.0};
    fetch(k_lo);
    stash(0);
    __syncthreads();
    int cur = 0;
    const int wr = (wv & 1) * (TM / 2), wc = (wv >> 1) * (TN / 2);
    for (int k0 = k_lo; k0 < k_hi; k0 += KC) {
        const bool more = k0 + KC < k_hi;
        if (more) fetch(k0 + KC);
#pragma unroll
        for (int kk = 0; kk < KC; kk += 4) {
            double ac[NC], br[MR];
#pragma unroll
            for (int jc = 0; jc < NC; ++jc) ac[jc] = sB[cur][kk + l4][wc + 16 * jc + l15];
#pragma unroll
            for (int ir = 0; ir < MR; ++ir) br[ir] = sA[cur][kk + l4][wr + 16 * ir + l15];
#pragma unroll
            for (int jc = 0; jc < NC; ++jc)
#pragma unroll
                for (int ir = 0; ir < MR; ++ir) acc[jc][ir] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[jc], br[ir], acc[jc][ir], 0, 0, 0);
        }
        if (more) stash(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    double* dst = PHASE == 0 ? T : X;
#pragma unroll
    for (int jc = 0; jc < NC; ++jc)
#pragma unroll
        for (int ir = 0; ir < MR; ++ir)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int c = c0 + wc + 16 * jc + l4 + 4 * reg;     // D[i = l4 + 4 reg -> column][j = l15 -> row]
                const int r = r0 + wr + 16 * ir + l15;
                if (r < mB) dst[(b0 + r) + (size_t)ldx * (a0 + c)] = PHASE == 0 ? acc[jc][ir][reg] : -acc[jc][ir][reg];
            }
}

// W = L21 X, written over L21 (option "sweep_w": the one-launch form of the wide levels' sweeps, k_sweep_fwd_w / k_sweep_bwd_w).  Row r
// of W depends on row r of L21 only, so a workgroup owns 64 boundary rows and walks the column blocks from the left:
//   W[r][c0 .. c0 + 127] = sum_{k >= c0} L21[r][k] X[k][c0 .. c0 + 127]      (X lower triangular),
// block c0 reads the entries of its rows in the columns >= c0 and then overwrites the columns c0 .. c0 + 127 -- which no later block
// reads.  fp64 MFMA, both operands staged through LDS 16 columns of k at a time (the scheme of k_xinv); runs on stream3 behind the
// level's k_xinv launches, beside the factorisation of the levels above.
constexpr int WT_M = 64, WT_N = 128;
__global__ void __launch_bounds__(256, 2)
k_w_inplace(FrontDev fd, const int* __restrict__ level_nodes, int first) {
    const int t = level_nodes[first + blockIdx.y];
    const int np = fd.npiv[t], nf = fd.nf[t], nb = nf - np;
    const int r0 = blockIdx.x * WT_M;
    if (np == 0 || r0 >= nb) return;
    const int ldp = ldp_of(nf), ldx = ldx_of(np);
    double* L = fd.P + fd.poff[t] + np;                   // L21: rows np.. of the pivot columns
    const double* X = fd.X + fd.xoff[t];
    constexpr int KC = 16, SA = WT_M + 16, SB = WT_N + 16;
    constexpr int QA = KC / 4, QB = WT_N / 16;
    __shared__ double sA[2][KC][SA];                      // sA[.][k][r] = L21[r0 + r][k]
    __shared__ double sB[2][KC][SB];                      // sB[.][k][c] = X[k][c0 + c]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int lr = tid & 63, kq = tid >> 6;
    const int kb = tid & 15, cb = tid >> 4;
    const bool rok = r0 + lr < nb;
    const double* arow = L + min(r0 + lr, nb - 1);
    const int wr = (wv & 1) * 32, wc = (wv >> 1) * 64;
    for (int c0 = 0; c0 < np; c0 += WT_N) {
        double pa[QA], pb[QB];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int q = 0; q < QA; ++q) {
                const int k = k0 + kq + 4 * q;
                const double v = arow[(size_t)ldp * min(k, np - 1)];
                pa[q] = (rok && k < np) ? v : 0.0;
            }
#pragma unroll
            for (int q = 0; q < QB; ++q) {
                const int k = k0 + kb, c = c0 + cb + 16 * q;
                pb[q] = (k < np && c < np && k >= c) ? X[k + (size_t)ldx * c] : 0.0;
            }
        };
        auto stash = [&](int buf) {
#pragma unroll
            for (int q = 0; q < QA; ++q) sA[buf][kq + 4 * q][lr] = pa[q];
#pragma unroll
            for (int q = 0; q < QB; ++q) sB[buf][kb][cb + 16 * q] = pb[q];
        };
        mfma_d4 acc[4][2];
#pragma unroll
        for (int jc = 0; jc < 4; ++jc)
#pragma unroll
            for (int ir = 0; ir < 2; ++ir) acc[jc][ir] = (mfma_d4){0.0, 0.0, 0.0, 0.0};
        fetch(c0);
        stash(0);
        __syncthreads();
        int cur = 0;
        for (int k0 = c0; k0 < np; k0 += KC) {
            const bool more = k0 + KC < np;
            if (more) fetch(k0 + KC);
#pragma unroll
            for (int kk = 0; kk < KC; kk += 4) {
                double ac[4], br[2];
#pragma unroll
                for (int jc = 0; jc < 4; ++jc) ac[jc] = sB[cur][kk + l4][wc + 16 * jc + l15];
#pragma unroll
                for (int ir = 0; ir < 2; ++ir) br[ir] = sA[cur][kk + l4][wr + 16 * ir + l15];
#pragma unroll
                for (int jc = 0; jc < 4; ++jc)
#pragma unroll
                    for (int ir = 0; ir < 2; ++ir) acc[jc][ir] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[jc], br[ir], acc[jc][ir], 0, 0, 0);
            }
            if (more) stash(cur ^ 1);
            __syncthreads();                              // after the last pass: every wave has read the block's own columns
            cur ^= 1;
        }
#pragma unroll
        for (int jc = 0; jc < 4; ++jc)
#pragma unroll
            for (int ir = 0; ir < 2; ++ir)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int c = c0 + wc + 16 * jc + l4 + 4 * reg;     // D[i = l4 + 4 reg -> column][j = l15 -> row]
                    const int r = r0 + wr + 16 * ir + l15;
                    if (r < nb && c < np) L[r + (size_t)ldp * c] = acc[jc][ir][reg];
                }
    }
}

}  // namespace femo
