// Max-displacement (KS) aggregate of the static state and its gradient (include/femo_hip.h: femo_set_disp_aggregate), gfx950, fp64.
//
// Displacement nodes are the P2 nodes i < nP2 whose translations are w[3 i .. 3 i + 2]; the mesh vertices are the first nn of them.  A
// node is selected when it belongs to a cell of the selected sub-domain and its kind is asked for (vertices only, or every node):
//   x_i = s |u_i|   (norm mode, s > 0)      or      x_i = s (d . u_i)   (direction mode, s != 0, d as given)
//   S = x_max + 1/rho log sum_i exp(rho (x_i - x_max)),    M = S / s,    p_i = exp(rho (x_i - S)),    sum_i p_i = 1
//   dM/du_i = p_i u_i / |u_i| (exactly 0 where |u_i| = 0: a subgradient)      or      dM/du_i = p_i d
// This is the project's own contract, pinned by tests/disp_aggregate_ref.py.
//   k_da_mask     one thread per cell: mask[node] = 1 for the nodes of the selected cells.  Plain stores of the same value, no atomics.
//   k_da_count    selected nodes of either kind, { vertices, all } (integer atomics: exact in any order); read back once per mask
//   k_da_value    one thread per node, coalesced reads of the three translations.  A selected node carries the pair
//                 (m, z) = (x_i, 1) of (max x, sum exp(rho (x - m))), an unselected one the empty pair (-inf, 0).  Pairs are merged over
//                 the wave by a butterfly, over the block's waves in wave order, one slot (m, z, count, non-finite nodes) per block.
//   k_da_combine  merges the slots in a fixed order (256 contiguous runs in block order, a butterfly over each wave, the waves in order)
//                 and writes res = { S, M, N, non-finite nodes } for the host and for the gradient kernel.  No float atomics anywhere.
//   k_da_grad     one thread per node: a selected node writes its own three entries, the shift S read from res on the device.  It
//                 writes nothing else: rotations, unselected nodes and whatever follows the displacement block keep the caller's zeros.
#pragma once
#include "disp_history.h"

namespace femo {

constexpr int DA_BLOCK = 256;      // threads per block of the node kernels: four waves

// the parameters of one slot as the kernels take them
struct DispAggDev {
    double rho, s, d[3];
    int dir;                       // 0: norm mode, 1: direction mode
    int nlim;                      // nodes below this index are of the kind asked for: nn (vertices) or nP2 (all)
};

// union of two pairs (m, z) = (max x, sum exp(rho (x - m))); z = 0 is the empty pair, whose m = -inf is never used in arithmetic
// (-inf - (-inf) would be a NaN)
__device__ __forceinline__ void da_merge(double& m, double& z, double m2, double z2, double rho) {
    if (z2 == 0.0) return;
    if (z == 0.0) { m = m2; z = z2; return; }
    const double mx = fmax(m, m2);
    z = z * exp(rho * (m - mx)) + z2 * exp(rho * (m2 - mx));
    m = mx;
}

__device__ __forceinline__ double da_x(const DispAggDev& p, double ux, double uy, double uz) {
    return p.dir ? p.s * (p.d[0] * ux + p.d[1] * uy + p.d[2] * uz) : p.s * sqrt(ux * ux + uy * uy + uz * uz);
}

__global__ void __launch_bounds__(256)
k_da_mask(int nel, int npc, int nP2, const int* __restrict__ cellp2, const int* __restrict__ ctag, int csel, unsigned char* __restrict__ mask) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nel || !(csel < 0 || (ctag && ctag[e] == csel))) return;
    for (int a = 0; a < npc; ++a) {
        const int i = cellp2[(size_t)a * nel + e];
        if (i >= 0 && i < nP2) mask[i] = 1;
    }
}

__global__ void __launch_bounds__(256)
k_da_count(int nP2, int nn, const unsigned char* __restrict__ mask, int* __restrict__ cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int a = i < nP2 && mask[i] ? 1 : 0, v = a && i < nn ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off, 64); v += __shfl_xor(v, off, 64); }
    if ((threadIdx.x & 63) == 0 && a) { atomicAdd(cnt, v); atomicAdd(cnt + 1, a); }
}

// part[4 b + {0, 1, 2, 3}] = (m, z, selected nodes, selected nodes with a non-finite translation) of block b
__global__ void __launch_bounds__(DA_BLOCK)
k_da_value(int nP2, DispAggDev p, const unsigned char* __restrict__ mask, const double* __restrict__ w, double* __restrict__ part) {
    __shared__ double s_m[DA_BLOCK / 64], s_z[DA_BLOCK / 64];
    __shared__ int s_n[DA_BLOCK / 64], s_bad[DA_BLOCK / 64];
    const int tid = threadIdx.x, i = blockIdx.x * DA_BLOCK + tid;
    double m = -INFINITY, z = 0.0;
    int n = 0, bad = 0;
    if (i < p.nlim && i < nP2 && mask[i]) {
        const double ux = w[3 * (size_t)i], uy = w[3 * (size_t)i + 1], uz = w[3 * (size_t)i + 2];
        m = da_x(p, ux, uy, uz);
        z = 1.0;
        n = 1;
        bad = isfinite(ux) && isfinite(uy) && isfinite(uz) ? 0 : 1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double m2 = shfl_xor_d(m, off), z2 = shfl_xor_d(z, off);
        da_merge(m, z, m2, z2, p.rho);
        n += __shfl_xor(n, off, 64);
        bad += __shfl_xor(bad, off, 64);
    }
    const int lane = tid & 63, wid = tid >> 6;
    if (lane == 0) { s_m[wid] = m; s_z[wid] = z; s_n[wid] = n; s_bad[wid] = bad; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < DA_BLOCK / 64; ++k) { da_merge(m, z, s_m[k], s_z[k], p.rho); n += s_n[k]; bad += s_bad[k]; }
        double* o = part + 4 * (size_t)blockIdx.x;
        o[0] = m; o[1] = z; o[2] = (double)n; o[3] = (double)bad;
    }
}

// res = { S, M = S / s, N, non-finite nodes }.  A fixed order: every thread merges a contiguous run of block slots in block order, a
// butterfly merges the runs of a wave, thread 0 the four waves in wave order (a serial merge of the 256 runs, two exp per step on one
// lane, took several times as long as the node pass: DESIGN.md).  The counts are small integers: exact in any order.
__global__ void __launch_bounds__(256)
k_da_combine(int nb, const double* __restrict__ part, double rho, double s, double* __restrict__ res) {
    __shared__ double s_m[4], s_z[4], s_n[4], s_bad[4];
    const int t = threadIdx.x, per = (nb + 255) / 256;
    double m = -INFINITY, z = 0.0, n = 0.0, bad = 0.0;
    for (int b = t * per; b < min(nb, (t + 1) * per); ++b) {
        const double* q = part + 4 * (size_t)b;
        da_merge(m, z, q[0], q[1], rho);
        n += q[2];
        bad += q[3];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double m2 = shfl_xor_d(m, off), z2 = shfl_xor_d(z, off);
        da_merge(m, z, m2, z2, rho);
        n += shfl_xor_d(n, off);
        bad += shfl_xor_d(bad, off);
    }
    if ((t & 63) == 0) { s_m[t >> 6] = m; s_z[t >> 6] = z; s_n[t >> 6] = n; s_bad[t >> 6] = bad; }
    __syncthreads();
    if (t == 0) {
        for (int k = 1; k < 4; ++k) { da_merge(m, z, s_m[k], s_z[k], rho); n += s_n[k]; bad += s_bad[k]; }
        const double S = z > 0.0 ? m + log(z) / rho : -INFINITY;
        res[0] = S;
        res[1] = S / s;
        res[2] = n;
        res[3] = bad;
    }
}

// out[3 i .. 3 i + 2] = dM/du_i of the selected nodes; every other entry of out is left as it is (the caller's zeros)
__global__ void __launch_bounds__(DA_BLOCK)
k_da_grad(int nP2, DispAggDev p, const unsigned char* __restrict__ mask, const double* __restrict__ w, const double* __restrict__ res,
          double* __restrict__ out) {
    const int i = blockIdx.x * DA_BLOCK + threadIdx.x;
    if (!(i < p.nlim && i < nP2 && mask[i])) return;
    const double S = res[0];
    const double ux = w[3 * (size_t)i], uy = w[3 * (size_t)i + 1], uz = w[3 * (size_t)i + 2];
    const double pi = exp(p.rho * (da_x(p, ux, uy, uz) - S));
    double gx, gy, gz;
    if (p.dir) {
        gx = pi * p.d[0]; gy = pi * p.d[1]; gz = pi * p.d[2];
    } else {
        const double r = sqrt(ux * ux + uy * uy + uz * uz);
        const double c = r > 0.0 ? pi / r : 0.0;
        gx = c * ux; gy = c * uy; gz = c * uz;
    }
    out[3 * (size_t)i] = gx; out[3 * (size_t)i + 1] = gy; out[3 * (size_t)i + 2] = gz;
}

}  // namespace femo
