// rs_sky_build.hip -- the sky's sampling tables on the device (rs_sky.h has their definition): a maximum pass, a row
// pass (one workgroup per sky row: cell weights from two staged texel rows, quantised, scanned) and a marginal pass
// (one workgroup scans the row totals).  Integer tables: the scans' order does not matter, and the sequential restatement
// (tests/cpp/sky_oracle.c or_sky_tables) gives the same words.
#include <hip/hip_runtime.h>
#include "rs_sky.h"

namespace rs {
namespace {

constexpr int kSkyBlock = 256;

// The weights of the cells [c0, c0 + 256) of sky row j, one per thread (0 past the row's end).  ts: the rgb sums of the
// texels [c0, c0 + 256] of rows j and j + 1 (tex_texel clamps both coordinates to the edge), staged once so that each
// texel is read from memory by one thread and from LDS by the two cells it is a corner of.
__device__ __forceinline__ float chunk_weight(const DevScene& S, int w, int j, float sin_row, int c0,
                                              float (*ts)[kSkyBlock + 1]) {
    __syncthreads();                                                 // the chunk before has been read
    for (int k = threadIdx.x; k < 2 * (kSkyBlock + 1); k += kSkyBlock) {
        const int r = k / (kSkyBlock + 1), c = k - r * (kSkyBlock + 1);
        const vec3 t = tex_texel(S, S.sky, c0 + c, j + r, false);
        ts[r][c] = (t.x + t.y) + t.z;
    }
    __syncthreads();
    const int l = threadIdx.x;
    if (c0 + l >= w) return 0.0f;
    return sky_weight((ts[0][l] + ts[0][l + 1]) + (ts[1][l] + ts[1][l + 1]), sin_row);
}

// Wmax, as the bits of a non-negative float (their unsigned order is the floats')
__global__ void __launch_bounds__(kSkyBlock) k_sky_max(DevScene S, int w, int h, uint32_t* wmax) {
    __shared__ float ts[2][kSkyBlock + 1];
    __shared__ uint32_t m;
    const int j = blockIdx.x;
    if (threadIdx.x == 0) m = 0u;
    const float sin_row = sky_sin_row(j, h);
    uint32_t mine = 0u;
    for (int c0 = 0; c0 < w; c0 += kSkyBlock) {
        const uint32_t b = __float_as_uint(chunk_weight(S, w, j, sin_row, c0, ts));
        mine = b > mine ? b : mine;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = __shfl_xor(mine, d);
        mine = o > mine ? o : mine;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(&m, mine);               // m = 0 is ordered by chunk_weight's barriers
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(wmax, m);
}

// Row j: q of every cell, the inclusive prefix sum into row_cdf, the total into row_tot.  A wave scans its 64 cells by
// shuffles, the four wave totals and the running carry of the chunks before go through LDS and a register.
__global__ void __launch_bounds__(kSkyBlock) k_sky_rows(DevScene S, int w, int h, const uint32_t* wmax, uint32_t* row_cdf,
                                                        uint32_t* row_tot) {
    __shared__ float ts[2][kSkyBlock + 1];
    __shared__ uint32_t wsum[kSkyBlock / 64];
    const int j = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float sin_row = sky_sin_row(j, h), Wmax = __uint_as_float(*wmax);
    uint32_t carry = 0u;                                             // the same in every thread
    for (int c0 = 0; c0 < w; c0 += kSkyBlock) {
        uint32_t v = sky_quant(chunk_weight(S, w, j, sin_row, c0, ts), Wmax);
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t n = __shfl_up(v, d);
            if (lane >= d) v += n;
        }
        if (lane == 63) wsum[wave] = v;                              // read below; rewritten after the next chunk's barriers
        __syncthreads();
        uint32_t off = 0u, tot = 0u;
        for (int k = 0; k < kSkyBlock / 64; ++k) {
            const uint32_t s = wsum[k];
            off += k < wave ? s : 0u;
            tot += s;
        }
        const int i = c0 + (int)threadIdx.x;
        if (i < w) row_cdf[(size_t)j * (size_t)w + (size_t)i] = carry + off + v;
        carry += tot;
    }
    if (threadIdx.x == 0) row_tot[j] = carry;
}

// the inclusive prefix sum of the h row totals, in uint64: one workgroup
__global__ void __launch_bounds__(kSkyBlock) k_sky_marginal(const uint32_t* row_tot, int h, uint64_t* marginal) {
    __shared__ uint64_t wsum[kSkyBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (int c0 = 0; c0 < h; c0 += kSkyBlock) {
        const int j = c0 + (int)threadIdx.x;
        unsigned long long v = j < h ? row_tot[j] : 0u;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long n = __shfl_up(v, d);
            if (lane >= d) v += n;
        }
        __syncthreads();                                             // the chunk before has read wsum
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        uint64_t off = 0, tot = 0;
        for (int k = 0; k < kSkyBlock / 64; ++k) {
            const uint64_t s = wsum[k];
            off += k < wave ? s : 0;
            tot += s;
        }
        if (j < h) marginal[j] = carry + off + v;
        carry += tot;
    }
}

}  // namespace

int build_sky_tables(const DevScene& S, int w, int h, hipStream_t st, uint32_t** row_cdf, uint64_t** marginal,
                     uint64_t* total, std::string& err) {
    *row_cdf = nullptr; *marginal = nullptr; *total = 0;
    if (w < 1 || h < 1 || w > kSkyMaxWidth || S.sky < 0) { err = "build_sky_tables: no sky, or one wider than 32768"; return -1; }
    uint32_t* scratch = nullptr;                                     // h row totals, then Wmax
    auto bail = [&](const char* what, hipError_t e) {
        err = std::string("build_sky_tables: ") + what + ": " + hipGetErrorString(e);
        hipStreamSynchronize(st);
        if (scratch) hipFree(scratch);
        if (*row_cdf) hipFree(*row_cdf);
        if (*marginal) hipFree(*marginal);
        *row_cdf = nullptr; *marginal = nullptr;
        return -1;
    };
    hipError_t e;
    if ((e = hipMalloc(&scratch, ((size_t)h + 1) * sizeof(uint32_t))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMalloc(row_cdf, (size_t)w * (size_t)h * sizeof(uint32_t))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMalloc(marginal, (size_t)h * sizeof(uint64_t))) != hipSuccess) return bail("hipMalloc", e);
    uint32_t* wmax = scratch + h;
    if ((e = hipMemsetAsync(wmax, 0, sizeof(uint32_t), st)) != hipSuccess) return bail("hipMemsetAsync", e);
    k_sky_max<<<h, kSkyBlock, 0, st>>>(S, w, h, wmax);
    k_sky_rows<<<h, kSkyBlock, 0, st>>>(S, w, h, wmax, *row_cdf, scratch);
    k_sky_marginal<<<1, kSkyBlock, 0, st>>>(scratch, h, *marginal);
    if ((e = hipGetLastError()) != hipSuccess) return bail("launch", e);
    if ((e = hipMemcpyAsync(total, *marginal + (h - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, st)) != hipSuccess)
        return bail("hipMemcpyAsync", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return bail("hipStreamSynchronize", e);
    hipFree(scratch);
    return 0;
}

}  // namespace rs
