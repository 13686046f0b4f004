// pc_util.hip -- small device utilities of the pair pipeline: the exclusive u32 prefix sum, a u32 gather, the shard assembly on the
// root, and the two test hooks (round6 probe, alignment-result unpack).  Restates of the reference only round(x, 6), through pc_round6.
#include "pc_pairs.h"

__global__ void k_round6_probe(const double* in, double* out, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = pc_round6(in[i]);
}
int pc_launch_round6_probe(const double* in, double* out, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_round6_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, out, n);
    return hipGetLastError() == hipSuccess ? PC_OK : PC_ERR_HIP;
}

// ---------------------------------------------------------------------------------
// Exclusive prefix sum of u32 (n elements).  2048 elements per workgroup, block sums
// scanned recursively.  Callers that need the total pass n+1 elements with in[n] = 0.
// ---------------------------------------------------------------------------------
#define SCAN_PER_BLOCK 2048

__global__ __launch_bounds__(256) void k_scan_block(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                     uint32_t* __restrict__ sums, int64_t n) {
    __shared__ uint32_t wsum[4];
    const int64_t base = (int64_t)blockIdx.x * SCAN_PER_BLOCK + (int64_t)threadIdx.x * 8;
    uint32_t v[8], tot = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[i] = (base + i < n) ? in[base + i] : 0u; tot += v[i]; }
    // wave inclusive scan of the per-thread totals
    uint32_t incl = tot;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { uint32_t y = __shfl_up(incl, o); if (lane >= o) incl += y; }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    uint32_t woff = 0;
    for (int i = 0; i < wv; ++i) woff += wsum[i];
    uint32_t run = woff + incl - tot;
#pragma unroll
    for (int i = 0; i < 8; ++i) { if (base + i < n) out[base + i] = run; run += v[i]; }
    if (threadIdx.x == 255 && sums) sums[blockIdx.x] = woff + incl;
}

__global__ __launch_bounds__(256) void k_scan_add(uint32_t* __restrict__ out, const uint32_t* __restrict__ sums, int64_t n) {
    const uint32_t add = sums[blockIdx.x];
    const int64_t base = (int64_t)blockIdx.x * SCAN_PER_BLOCK + (int64_t)threadIdx.x * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) if (base + i < n) out[base + i] += add;
}

int64_t pc_scan_tmp_elems(int64_t n) {
    int64_t tot = 0;
    while (n > SCAN_PER_BLOCK) { n = (n + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK; tot += n; }
    return tot + 1;
}

int pc_scan_exclusive_u32(const uint32_t* in, uint32_t* out, int64_t n, uint32_t* tmp, int64_t tmp_elems, hipStream_t st) {
    if (n <= 0) return PC_OK;
    const int64_t nb = (n + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK;
    if (nb == 1) {
        hipLaunchKernelGGL(k_scan_block, dim3(1), dim3(256), 0, st, in, out, (uint32_t*)nullptr, n);
    } else {
        if (tmp_elems < nb) { pc_set_error("scan: temp too small"); return PC_ERR_ARG; }
        hipLaunchKernelGGL(k_scan_block, dim3((unsigned)nb), dim3(256), 0, st, in, out, tmp, n);
        int rc = pc_scan_exclusive_u32(tmp, tmp, nb, tmp + nb, tmp_elems - nb, st);
        if (rc != PC_OK) return rc;
        hipLaunchKernelGGL(k_scan_add, dim3((unsigned)nb), dim3(256), 0, st, out, tmp, n);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("scan launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}

__global__ void k_gather_u32(const uint32_t* __restrict__ src, const int32_t* __restrict__ idx, uint32_t* __restrict__ dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}
int pc_launch_gather_u32(const uint32_t* src, const int32_t* idx, uint32_t* dst, int n, hipStream_t st) {
    hipLaunchKernelGGL(k_gather_u32, dim3((n + 63) / 64), dim3(64), 0, st, src, idx, dst, n);
    return hipGetLastError() == hipSuccess ? PC_OK : PC_ERR_HIP;
}

// ---------------------------------------------------------------------------------
// Shard assembly on the root: gathered[r][lbase_r(k) + s] -> condensed(s, t).
// The boustrophedon deal has closed forms: round j = t / world, rank r = pos or
// world-1-pos, and lbase_r(k) = world*k(k-1)/2 + r*ceil(k/2) + (world-1-r)*floor(k/2).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_assemble(const double* __restrict__ gathered, int world, int64_t stride, int N,
                                                   double* __restrict__ out) {
    const int s = blockIdx.y;
    const int t = s + 1 + blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    const int j = t / world, pos = t % world;
    const int r = (j & 1) ? world - 1 - pos : pos;
    const int64_t k = j;
    const int64_t lbase = (int64_t)world * (k * (k - 1) / 2) + (int64_t)r * ((k + 1) / 2) + (int64_t)(world - 1 - r) * (k / 2);
    out[(int64_t)s * N - (int64_t)s * (s + 1) / 2 + (t - s - 1)] = gathered[(int64_t)r * stride + lbase + s];
}
// Same for an arbitrary deal: t_rank[t] owns target t, whose pairs start at t_lbase[t] inside that rank's shard.
__global__ __launch_bounds__(256) void k_assemble_table(const double* __restrict__ gathered, int64_t stride, int N,
                                                         const int32_t* __restrict__ t_rank, const int64_t* __restrict__ t_lbase,
                                                         double* __restrict__ out) {
    const int s = blockIdx.y;
    const int t = s + 1 + blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    out[(int64_t)s * N - (int64_t)s * (s + 1) / 2 + (t - s - 1)] = gathered[(int64_t)t_rank[t] * stride + t_lbase[t] + s];
}
int pc_launch_assemble_table(const double* gathered, int64_t stride, int N, const int32_t* t_rank, const int64_t* t_lbase, double* out, hipStream_t st) {
    if (N <= 1) return PC_OK;
    dim3 grid((N + 255) / 256, N - 1);
    hipLaunchKernelGGL(k_assemble_table, grid, dim3(256), 0, st, gathered, stride, N, t_rank, t_lbase, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_assemble_table launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}

int pc_launch_assemble(const double* gathered, int world, int64_t stride, int N, double* out, hipStream_t st) {
    if (N <= 1) return PC_OK;
    dim3 grid((N + 255) / 256, N - 1);
    hipLaunchKernelGGL(k_assemble, grid, dim3(256), 0, st, gathered, world, stride, N, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_assemble launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}

// (n_ident, aln_len) -> (n_ident, n_diag) for the pc_align_pairs test hook
__global__ void k_unpack_res(const uint2* __restrict__ res, const int32_t* __restrict__ la_plus_lb,
                             int32_t* __restrict__ n_ident, int32_t* __restrict__ n_diag, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    n_ident[i] = (int32_t)res[i].x;
    n_diag[i] = la_plus_lb[i] - (int32_t)res[i].y;
}
int pc_launch_unpack_res(const uint2* res, const int32_t* la_plus_lb, int32_t* n_ident, int32_t* n_diag, int64_t n, hipStream_t st) {
    if (n <= 0) return PC_OK;
    hipLaunchKernelGGL(k_unpack_res, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, res, la_plus_lb, n_ident, n_diag, n);
    return hipGetLastError() == hipSuccess ? PC_OK : PC_ERR_HIP;
}
