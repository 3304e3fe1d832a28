// rs_sky.h -- the equirect sky as a sampled light: the tables' definition, their builder's entry
// (rs_sky_build.hip) and the device functions the unbiased sky estimator of rs_path.h samples and weighs with.
//
// Radiance function: sky_texel (rs_texture.h) -- the sky texture of w x h texels read bilinearly between integer texel
// coordinates, clamped to the edge, at px = x w, py = acos(z) / pi h.  The sampling distribution is piecewise constant
// over the unit cells (i, j) of (px, py) space, which are the bilinear patches of that function:
//   W(i, j) = max(0, rgb sum of the four corner texels (i | i + 1, j | j + 1)) * sin(pi (j + 1/2) / h)
// A parallel scan and a sequential one add floats in different orders, so the tables are integers:
//   Wmax    = max W (a maximum is exact in any order)
//   q(i, j) = W == 0 ? 0 : min((uint32)(W / Wmax * 65535.0f) + 1, 65536)
//   row_cdf = per row the inclusive prefix sum of q, uint32 (w <= 32768: a row total is < 2^32)
//   marginal = the inclusive prefix sum of the row totals, uint64
// Restated sequentially in tests/cpp/sky_oracle.c (or_sky_tables); the device tables equal it exactly.
#pragma once
#include <string>
#include "rs_texture.h"

namespace rs {

// The tables as a kernel argument of their own: DevScene, a by-value argument of every hot kernel, stays as it is.
struct SkyLight {
    const uint32_t* row_cdf;   // h rows of w
    const uint64_t* marginal;  // h
    int w, h;
    uint64_t total;            // marginal[h - 1]; 0: nothing to sample (no tables, or a sky without light)
};
constexpr int kSkyMaxWidth = 32768;
constexpr float kTwoPiSq = 19.7392088021787172376689819991f;   // 2 pi^2: d(px, py) -> solid angle is 2 pi^2 sin / (w h)

// ---- rs_sky_build.hip
// The tables of the sky S.sky (w x h texels) on stream st: new device allocations owned by the caller, *total read
// back (synchronises st).  0, or -1 with err set.
int build_sky_tables(const DevScene& S, int w, int h, hipStream_t st, uint32_t** row_cdf, uint64_t** marginal,
                     uint64_t* total, std::string& err);

__device__ __forceinline__ float sky_weight(float rgb_sum, float sin_row) {
    const float s = rgb_sum > 0.0f ? rgb_sum : 0.0f;                // NaN, negative: 0
    const float W = s * sin_row;
    return W > 0.0f ? W : 0.0f;
}
__device__ __forceinline__ float sky_sin_row(int j, int h) { return rs_sinf(kPi * ((float)j + 0.5f) / (float)h); }
__device__ __forceinline__ uint32_t sky_quant(float W, float Wmax) {
    if (!(W > 0.0f)) return 0u;
    float r = W / Wmax * 65535.0f;
    if (!(r >= 0.0f)) r = 0.0f;                                     // inf / inf
    if (r > 65535.0f) r = 65535.0f;
    return (uint32_t)r + 1u;
}

// solid-angle density of the cell of weight q at polar sine sin_t
__device__ __forceinline__ float sky_cell_pdf(const SkyLight& K, uint32_t q, float sin_t) {
    if (!(sin_t > 0.0f)) return 0.0f;
    const float pc = (float)((double)q / (double)K.total);
    return pc * ((float)K.w * (float)K.h) / (kTwoPiSq * sin_t);
}
// the first k of [0, n) with cdf[k] > t, for t < cdf[n - 1]
template <class C>
__device__ __forceinline__ int sky_upper(const C* cdf, int n, uint64_t t) {
    int lo = 0, len = n;
    while (len > 0) {
        const int half = len >> 1;
        if ((uint64_t)cdf[lo + half] <= t) { lo += half + 1; len -= half + 1; }
        else len = half;
    }
    return lo < n ? lo : n - 1;
}

// One sky sample from two draws (K.total > 0): row by the marginal, column by the row's CDF, the position inside the
// cell from the two remainders.  Radiance from the sampled texel coordinates directly: no inverse trigonometry.
struct SkySample { vec3 dir, L; float pdf; };
__device__ __forceinline__ SkySample sky_sample(const DevScene& S, const SkyLight& K, float u_row, float u_col) {
    uint64_t t = (uint64_t)((double)u_row * (double)K.total);
    if (t >= K.total) t = K.total - 1;
    const int j = sky_upper(K.marginal, K.h, t);
    const uint64_t m0 = j ? K.marginal[j - 1] : 0;
    const uint64_t rt = K.marginal[j] - m0;                         // > t - m0 >= 0
    const float fy = (float)((double)(t - m0) / (double)rt);
    const uint32_t* row = K.row_cdf + (size_t)j * (size_t)K.w;
    uint64_t t2 = (uint64_t)((double)u_col * (double)rt);
    if (t2 >= rt) t2 = rt - 1;
    const int i = sky_upper(row, K.w, t2);
    const uint32_t c0 = i ? row[i - 1] : 0u;
    const uint32_t q = row[i] - c0;                                 // > t2 - c0 >= 0
    const float fx = (float)((double)(t2 - c0) / (double)q);
    const float px = (float)i + fx, py = (float)j + fy;
    const float th = py / (float)K.h * kPi, ph = (px / (float)K.w - 0.5f) * (2.0f * kPi);
    float st, ct, sp, cp;
    rs_sincosf(th, &st, &ct);
    rs_sincosf(ph, &sp, &cp);
    SkySample r;
    r.dir = mk(st * cp, st * sp, ct);
    r.pdf = sky_cell_pdf(K, q, st);
    r.L = tex_bilinear_px(S, S.sky, px, py, false);
    return r;
}

__device__ __forceinline__ int sky_cell_of(float p, int n) {        // floor, clamped to the last cell; NaN: 0
    if (!(p >= 0.0f)) return 0;
    if (p >= (float)n) return n - 1;
    return (int)p;
}
// The sky along wi, as sky_texel gives it, and the density the sky sample has on wi: the cell from sky_texel's own
// texel coordinates
__device__ __forceinline__ vec3 sky_lookup(const DevScene& S, const SkyLight& K, vec3 wi, float& p_sky) {
    float x, y;
    sky_uv(wi, x, y);
    const float pxc = x * (float)K.w, pyc = (1.0f - y) * (float)K.h;
    const int i = sky_cell_of(pxc, K.w), j = sky_cell_of(pyc, K.h);
    const uint32_t* row = K.row_cdf + (size_t)j * (size_t)K.w;
    const uint32_t q = row[i] - (i ? row[i - 1] : 0u);
    p_sky = sky_cell_pdf(K, q, sqrtf(gmax(0.0f, 1.0f - wi.z * wi.z)));
    return tex_bilinear_px(S, S.sky, pxc, pyc, false);
}

}  // namespace rs
