// rs_path_unbiased.h -- the unbiased NEE + MIS path tracer: a ground truth that equals the light.
//
// rs_mis.h and rs_path.h restate the reference's estimators bit for bit, three biases included.
// This is the textbook estimator over the same material model (MisSurf: Phong for PHONG/DIELECTRIC, Lambert
// otherwise), free of the reference's structure.  Per path vertex: one light sample with its shadow ray
// (mis_light_part, unchanged) and one BRDF sample whose ray does both jobs -- an emitter it finds is the BRDF
// strategy's direct estimate (Le * power weight, resolved where the ray was traced), any other surface is the next
// vertex.  What differs from k_path_nee:
//   - the BRDF sample carries the full BRDF (mis_brdf) over the mixture pdf, not the sampled lobe's;
//   - its ray starts at the surface point h.pos, where the shadow rays start, so both MIS strategies measure a
//     light point from one origin and their weights sum to one.  FrameConst::normal_off (rs_frame_params::
//     normal_offset) is NOT used by this estimator; self-hits are kept off by tnear = FLT_MIN + tnear_offset;
//   - Russian roulette (bounce > 5, q = min(max(maxc Kd, maxc Ks) of the record, 1)) is drawn after the emitter
//     test and divides the whole return of the vertex, direct part included;
//   - one closest-hit ray per vertex instead of two: two walks per iteration, not three.
// RNG: pass kPassMis, one stream per pixel, draws in the recursion's order over the samples.  The estimator's
// definition is the recursion in tests/cpp/path_unbiased_oracle.c or_render_path_unbiased; this kernel equals it
// bit for bit.
//
// Shape of k_path_nee (rs_path.h): one wave-uniform loop, every ray query made by the whole wave with a
// predicate, per-lane walks inside the loop, lanes refilled from the cached camera vertex when their path ends,
// the finished path folded deepest level first from level-major LDS records -- rec[(l * 8 + f) * 256 + t], no
// barrier, (max_bounces + 1) * 8 KiB per workgroup.  A record is (Ld / q, f_r, |cos|, pdf * q).
#pragma once
#include "rs_path.h"

namespace rs {

// the draws of mis_sample (evaluateLightingGI), wi and the mixture pdf; f_r is the full BRDF on wi
__device__ __forceinline__ vec3 mis_sample_full(const MisSurf& h, Rng& rng, vec3& f_r, float& pdf) {
    bool diffuse = true;
    if (h.phong) diffuse = rng.range(0.0f, h.maxD + h.maxS) < h.maxD;
    vec3 wi;
    if (diffuse) wi = cosine_sample(h.n, rng);
    else wi = lobe_sample(h.wr, h.shin, rng);
    const LobePow lp = mis_lobe_pow(h, wi);                        // one power for the pdf and the BRDF
    pdf = mis_pdf_for(h, wi, lp);
    f_r = mis_brdf(h, lp);
    if (dot(h.n, wi) < 0) f_r = mk(0, 0, 0);
    return wi;
}

template <int T>
__global__ void __launch_bounds__(kPathBlock) k_path_unbiased(DevScene S, FrameConst F, PathConst Q, float* fb, CountSlot C) {
    extern __shared__ __attribute__((aligned(16))) float path_rec[];
    constexpr int TL = T | TRAV_LANE;               // past the camera vertex every ray is incoherent
    float* const rec = path_rec + threadIdx.x;
    int x, y;
    const bool in = pixel_of(F, F.y0, F.y1, x, y);
    const uint64_t t0 = wave_clock();
    const uint32_t pix = (uint32_t)y * (uint32_t)F.W + (uint32_t)x;
    uint32_t rays = in ? 1u : 0u;
    vec3 dc = mk((float)x - (float)F.W / 2.0f, (float)F.H / 2.0f - (float)y, -F.cam.focal);
    const float* m = F.inv_view;
    vec3 d = normalize(mk(m[0] * dc.x + m[3] * dc.y + m[6] * dc.z, m[1] * dc.x + m[4] * dc.y + m[7] * dc.z,
                          m[2] * dc.x + m[5] * dc.y + m[8] * dc.z));
    SurfHit hi = intersect<T>(S, in, F.cam.pos, d, FLT_MIN + 0.01f);
    MatRec mr = load_mat(S, hi.mat);
    const bool surf = in && hi.hit && !any_pos(mr.le);               // an emitter at the camera vertex -> Le
    vec3 px = hi.hit ? mr.le : (F.use_sky ? sky_texel(S, d) : F.bg);  // miss: sky or bgColor
    const MisSurf h0 = path_surf(S, hi, mr, d, surf);                // the camera vertex, once per pixel
    Rng rng; rng.init(F.seed, F.frame, kPassMis, pix);
    vec3 acc = mk(0, 0, 0);
    MisSurf h = h0;                                                  // the vertex this iteration handles
    int k = surf ? 0 : Q.spp, b = 0;                                 // sample and bounce of that vertex
    float q = 1.0f;                                                  // its roulette survival probability
    // every iteration moves every live lane one vertex on and a sample has at most max_bounces + 1 of them, so
    // the bound is never what ends the loop; it is there so that nothing can spin
    const uint32_t cap = (uint32_t)Q.spp * (uint32_t)(Q.max_bounces + 1);
    for (uint32_t it = 0; it < cap; ++it) {
        const bool live = k < Q.spp;
        if (__ballot(live) == 0) break;
        vec3 Ld = mk(0, 0, 0);
        if (Q.di) Ld = mk(0, 0, 0) + mis_light_part<TL>(S, F, h, live, rng, rays);
        Ld = dvs(sanitize(Ld), q);
        vec3 f_r;
        float pdf;
        const vec3 wi = mis_sample_full(h, rng, f_r, pdf);           // always drawn
        const bool last = !Q.gi || b + 1 > Q.max_bounces;            // the next hit counts as an emitter only
        const bool go = live && !(last && !Q.di);
        rays += go ? 1u : 0u;
        const SurfHit nx = intersect<TL>(S, go, h.pos, wi, FLT_MIN + F.tnear_off);   // from where the shadow rays start
        if (live) {
            float* r = rec + b * (kPathRec * kPathBlock);
            r[0 * kPathBlock] = Ld.x; r[1 * kPathBlock] = Ld.y; r[2 * kPathBlock] = Ld.z;
            r[3 * kPathBlock] = f_r.x; r[4 * kPathBlock] = f_r.y; r[5 * kPathBlock] = f_r.z;
            r[6 * kPathBlock] = fabsf(dot(wi, h.n));
            r[7 * kPathBlock] = pdf * q;
        }
        MatRec mx = load_mat(S, nx.mat);
        vec3 R = mk(0, 0, 0);                                        // what the ray brings back
        bool more = false;                                           // the path goes on at the next hit
        float qx = 1.0f;
        if (go && !nx.hit && !last) R = F.use_sky ? sky_texel(S, wi) : F.bg;
        if (go && nx.hit) {
            if (any_pos(mx.le)) {                                    // the BRDF strategy's direct estimate
                if (Q.di) {
                    const vec3 le = mx.le;
                    vec3 ny = nx.normal;
                    if (S.texd) apply_maps(S, nx, mx, ny, true);
                    vec3 ld = nx.point - h.pos;
                    float r2 = dot(ld, ld);
                    ld = normalize(ld);
                    float cY = gmax(dot(-ld, ny), 0.0f);
                    float amf = cY / r2;
                    float w = mis_power(pdf * amf, emis_pdf_brdf(S, nx.emis_id));
                    R = le * w;
                }
            } else if (!last) {
                const bool rr = b + 1 > 5 && Q.rr;
                bool cut = false;
                if (rr) {                                            // the draw is made only under roulette
                    qx = gmin(gmax(maxc(mx.kd), maxc(mx.ks)), 1.0f);  // the record's colours, not the mapped ones
                    cut = qx <= rng.range(0.0f, 1.0f);
                }
                more = !cut;
            }
        }
        const MisSurf hx = path_surf(S, nx, mx, wi, more);
        if (live && more) { h = hx; ++b; q = qx; }
        if (live && !more) {
            for (int l = b; l >= 0; --l) {
                const float* r = rec + l * (kPathRec * kPathBlock);
                const vec3 ld = mk(r[0 * kPathBlock], r[1 * kPathBlock], r[2 * kPathBlock]);
                const vec3 fr = mk(r[3 * kPathBlock], r[4 * kPathBlock], r[5 * kPathBlock]);
                const vec3 li = sanitize(dvs((R * fr) * r[6 * kPathBlock], r[7 * kPathBlock]));
                R = li + ld;
            }
            acc = acc + R;
            ++k; b = 0; h = h0; q = 1.0f;
        }
    }
    if (surf) px = dvs(acc, (float)Q.spp);
    px = sanitize(px);
    if (in) store_rgb(fb, pix, px);
    count_rays(C, rays, in ? 1u : 0u, t0, y);
}

}  // namespace rs
