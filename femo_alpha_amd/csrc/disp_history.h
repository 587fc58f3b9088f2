// Max-displacement (KS) aggregate of the transient history and its gradient, gfx950, fp64.
//
//   x_k = |s| |w_k|,   M = ( x_max + 1/rho log sum_k exp(rho (x_k - x_max)) ) / s,   dM/dw_k = sign(s) sign(w_k) exp(rho (x_k - s M))
//
// over the selected entries k of the whole history W (levels x ndof, level-major): every entry (components = all) or the first
// ndof_u of every level (the mid-surface displacement).  This is our reading of the lpc example's
// max_disp = csdl.maximum(csdl.absolute(s W), rho) / s (ex_lpc_gust_response_opt.py:457-459, 770-772).  The kernels work in
// u_k = rho |s| |w_k| and carry pairs (m, z) = (max u, sum exp(u - m)):
//   k_disp_ks_partial  grid (blocks per level, levels): every block takes a contiguous run of its level's row, each thread reads
//                      16-byte pairs at a stride of the block (8-byte entries when ndof is odd), keeps its own (m, z) with ONE exp
//                      per entry, and the pairs are merged across the wave (butterfly of shuffles) and the waves (LDS, in wave
//                      order).  part[(l nbx + b) 3 + {0, 1, 2}] = (m, z, non-finite entries) -- no atomics.
//   k_disp_ks_combine  one block: the block pairs of every level in block order -> the level's pair and shift m + log z
//                      (= rho s M_l), then the levels in level order -> the total.  Bitwise repeatable.
//   k_disp_ks_grad     dM/dW = sign(s) sign(w) exp(u - shift) of a chunk of levels, the shift read from the combine's result on
//                      the device; zero where w = 0 and on the entries the selection leaves out.  Every exponent is <= 0.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace femo {

// (m, z) of the union of two sets; z = 0 is the empty set (m then carries no meaning)
__device__ __forceinline__ void ks_merge(double& m, double& z, double m2, double z2) {
    if (z2 == 0.0) return;
    if (z == 0.0) { m = m2; z = z2; return; }
    const double mx = fmax(m, m2);
    z = z * exp(m - mx) + z2 * exp(m2 - mx);
    m = mx;
}

// one entry into a thread's running pair: one exp whichever side of the running maximum it falls
__device__ __forceinline__ void ks_push(double& m, double& z, int& bad, double w, double c) {
    bad += isfinite(w) ? 0 : 1;
    const double u = c * fabs(w);
    const double d = u - m;                     // z = 0 at the start: m = 0, d >= 0, z becomes 1
    const double e = exp(-fabs(d));
    z = d > 0.0 ? z * e + 1.0 : z + e;
    m = d > 0.0 ? u : m;
}

__device__ __forceinline__ double shfl_xor_d(double v, int mask) {
    const int lo = __shfl_xor(__double2loint(v), mask, 64), hi = __shfl_xor(__double2hiint(v), mask, 64);
    return __hiloint2double(hi, lo);
}

template <bool VEC>
__global__ void __launch_bounds__(256)
k_disp_ks_partial(const double* __restrict__ H, int64_t ldh, int64_t ncols, double c, double* __restrict__ part) {
    __shared__ double s_m[4], s_z[4];
    __shared__ int s_bad[4];
    const int l = blockIdx.y, nbx = gridDim.x, b = blockIdx.x, tid = threadIdx.x;
    const double* row = H + (size_t)l * ldh;
    double m = 0.0, z = 0.0;
    int bad = 0;
    if (VEC) {                                  // ldh even: every row starts 16-byte aligned
        const int64_t nv = ncols >> 1, per = (nv + nbx - 1) / nbx;
        const int64_t lo = min(nv, (int64_t)b * per), hi = min(nv, lo + per);
        const double2* r2 = reinterpret_cast<const double2*>(row);
        for (int64_t v = lo + tid; v < hi; v += 4 * 256) {
            double2 a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = v + k * 256 < hi ? r2[v + k * 256] : make_double2(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (v + k * 256 < hi) { ks_push(m, z, bad, a[k].x, c); ks_push(m, z, bad, a[k].y, c); }
        }
        if ((ncols & 1) && b == nbx - 1 && tid == 0) ks_push(m, z, bad, row[ncols - 1], c);
    } else {
        const int64_t per = (ncols + nbx - 1) / nbx;
        const int64_t lo = min(ncols, (int64_t)b * per), hi = min(ncols, lo + per);
        for (int64_t v = lo + tid; v < hi; v += 4 * 256) {
            double a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = v + k * 256 < hi ? row[v + k * 256] : 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (v + k * 256 < hi) ks_push(m, z, bad, a[k], c);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double m2 = shfl_xor_d(m, off), z2 = shfl_xor_d(z, off);
        bad += __shfl_xor(bad, off, 64);
        ks_merge(m, z, m2, z2);
    }
    const int lane = tid & 63, wid = tid >> 6;
    if (lane == 0) { s_m[wid] = m; s_z[wid] = z; s_bad[wid] = bad; }
    __syncthreads();
    if (tid == 0) {
        double bm = s_m[0], bz = s_z[0];
        int bb = s_bad[0];
        for (int i = 1; i < 4; ++i) { ks_merge(bm, bz, s_m[i], s_z[i]); bb += s_bad[i]; }
        double* p = part + ((size_t)l * nbx + b) * 3;
        p[0] = bm; p[1] = bz; p[2] = (double)bb;
    }
}

// res: [0, L) shift m_l + log z_l of level l | [L, 2L) non-finite entries of level l | [2L, 3L) m_l | [3L, 4L) z_l |
//      4L: shift of the whole history | 4L + 1: its non-finite entries
__global__ void __launch_bounds__(256)
k_disp_ks_combine(int levels, int nbx, const double* __restrict__ part, double* __restrict__ res) {
    for (int l = threadIdx.x; l < levels; l += blockDim.x) {
        double m = 0.0, z = 0.0, bad = 0.0;
        for (int b = 0; b < nbx; ++b) {
            const double* p = part + ((size_t)l * nbx + b) * 3;
            ks_merge(m, z, p[0], p[1]);
            bad += p[2];
        }
        res[l] = m + log(z);
        res[levels + l] = bad;
        res[2 * levels + l] = m;
        res[3 * levels + l] = z;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = 0.0, z = 0.0, bad = 0.0;
        for (int l = 0; l < levels; ++l) {
            ks_merge(m, z, res[2 * levels + l], res[3 * levels + l]);
            bad += res[levels + l];
        }
        res[4 * levels] = m + log(z);
        res[4 * levels + 1] = bad;
    }
}

// out row j of the chunk (level l0 + blockIdx.y) = dM/dw of entry j (zero for j >= ncols); shift = res[4 levels] of the combine
template <bool VEC>
__global__ void __launch_bounds__(256)
k_disp_ks_grad(const double* __restrict__ H, int64_t ldh, int64_t ncols, int l0, double c, double sgn, const double* __restrict__ shift,
               double* __restrict__ out) {
    const double sh = *shift;
    const double* row = H + (size_t)(l0 + blockIdx.y) * ldh;
    double* o = out + (size_t)blockIdx.y * ldh;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    auto g = [&](double w, int64_t j) {
        return j < ncols && w != 0.0 ? sgn * copysign(1.0, w) * exp(c * fabs(w) - sh) : 0.0;
    };
    if (VEC) {
        const double2* r2 = reinterpret_cast<const double2*>(row);
        double2* o2 = reinterpret_cast<double2*>(o);
        for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < (ldh >> 1); v += stride) {
            const double2 w = r2[v];
            o2[v] = make_double2(g(w.x, 2 * v), g(w.y, 2 * v + 1));
        }
    } else {
        for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ldh; j += stride) o[j] = g(row[j], j);
    }
}

}  // namespace femo
