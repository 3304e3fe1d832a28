// rs_path.h -- the NEE path tracers: the global-illumination ground truths, one kernel for
// the three estimators (k_path's E; the third, the unbiased one under a sky, is described at the kernel and in DESIGN.md
// §3.31, its checker is spath_L in tests/cpp/sky_oracle.c).  The reference's:
//
// SimpleGuiDX11::produceStandard (pg/simpleguidx11.cpp:336-357) driving NEEPathIntegrator::integrateImpl2
// (pg/NEEPathIntegrator.cpp:72-131) with calcGI on: at every path vertex the MIS direct estimate of rs_mis.h
// (one BRDF ray, one light sample with its shadow ray) plus one BRDF-sampled continuation ray, up to
// RenderParams::maxBounceCount bounces, Russian roulette on max(maxc(Kd), maxc(Ks)) of the material record at
// bounce > 5; an emitter counts only at the camera vertex (next-event estimation).  Material model of rs_mis.h
// (MisSurf: Phong for PHONG/DIELECTRIC, Lambert otherwise), so this image, the MIS image and the ReSTIR image
// estimate the same scene.  RNG: pass kPassMis, one stream per pixel, draws in the recursion's order over the
// samples -- with calc_gi off the draws, and the frame, are k_direct_mis's.  Restated as the recursion path_L in
// tests/cpp/path_oracle.c (or_render_path); the unbiased estimator is defined by upath_L there (or_render_path_unbiased).
// The kernel equals both bit for bit.
//
// The recursion is unrolled into one wave-uniform loop.  sanitize() between the levels is not linear, so a
// forward throughput product would give other floats: every vertex of the path in flight leaves an 8-float
// record (Ld, f_r, |cos|, pdf * q) and the finished path is folded deepest level first, exactly as the return
// statements would.  The records live in dynamic LDS, level-major: field f of level l of thread t at
// rec[(l * 8 + f) * 256 + t] -- consecutive lanes on consecutive banks, every thread in its own column, so the
// loop needs no barrier; (max_bounces + 1) * 8 KiB per workgroup.
//
// One iteration handles one vertex of every live lane: direct part, continuation sample, next closest hit.  A
// lane whose path ended (miss, emitter, roulette, bounce limit) folds, adds to its accumulator and takes its
// next sample from the cached camera vertex in the next iteration instead of idling until the wave's longest
// path ends; the per-pixel streams make the result independent of that schedule.
#pragma once
#include "rs_mis.h"
#include "rs_sky.h"

namespace rs {

struct PathConst { int spp, max_bounces, rr, di, gi; };
constexpr int kPathRec = 8;                        // floats per vertex record
constexpr int kPathBlock = 256;                    // threads per workgroup = columns of the record array

// the MisSurf of a path vertex reached along d: all maps applied, wr = reflect(d, n), 1/I_M for Phong.  calc_I_M
// (the double-precision incomplete beta, the largest callee of the loop) stays the one out-of-line copy every
// kernel of the library calls, as rs_libm.h's pow core, so its registers are not the loop's; a wrapper of its
// own around it only added a 16-byte call frame in scratch.
__device__ __forceinline__ MisSurf path_surf(const DevScene& S, const SurfHit& hi, MatRec mr, vec3 d, bool on) {
    vec3 hn = hi.normal;
    if (S.texd && hi.hit) apply_maps(S, hi, mr, hn, false);
    MisSurf h;
    h.pos = hi.point; h.n = hn; h.kd = mr.kd; h.ks = mr.ks; h.shin = mr.shin;
    h.phong = is_phong(mr.type);
    h.maxD = maxc(h.kd); h.maxS = maxc(h.ks);
    h.pf = h.maxD / (h.maxD + h.maxS);
    h.wr = normalize(reflect(d, h.n));
    h.i_m = 0.0f;
    if (on && h.phong) h.i_m = 1.0f / calc_I_M(dot(-d, h.n), h.shin);
    return h;
}

// The sky strategy's direct estimate at h (kEstUnbiasedSky): one sky sample from two draws, an any-hit ray from h.pos
// with no far end, the power heuristic against the BRDF strategy's density on the sampled direction.  The emitters'
// counterpart is mis_light_part; the two integrate disjoint sets of directions.
template <int T>
__device__ __forceinline__ vec3 sky_light_part(const DevScene& S, const FrameConst& F, const SkyLight& K, const MisSurf& h,
                                               bool alive, Rng& rng, uint32_t& rays) {
    const float u_row = rng.range(0.0f, 1.0f), u_col = rng.range(0.0f, 1.0f);
    const SkySample s = sky_sample(S, K, u_row, u_col);
    const float cI = gmax(dot(s.dir, h.n), 0.0f);
    const bool ok = alive && s.pdf > 0.0f && cI > 0;
    rays += ok ? 1u : 0u;
    const bool occ = trace_any<T>(S, ok, h.pos, s.dir, FLT_MIN + F.tnear_off, FLT_MAX);
    if (!ok || occ) return mk(0, 0, 0);
    const LobePow lp = mis_lobe_pow(h, s.dir);
    const float w = mis_power(s.pdf, mis_pdf_for(h, s.dir, lp));
    if (!(w > 0.0f)) return mk(0, 0, 0);
    return dvs(((s.L * w) * mis_brdf(h, lp)) * cI, s.pdf);
}

template <int T, int E, bool kRows = false>                         // kRows: as k_direct_mis's
__global__ void __launch_bounds__(kPathBlock) k_path(DevScene S, FrameConst F, PathConst Q, float* fb, CountSlot C,
                                                       RowSet R, SkyLight K) {
    // E = kEstReference restates the reference's estimator bit for bit, three biases included.
    // E = kEstUnbiased is the textbook estimator over the same material model, free of the reference's structure: per
    // vertex one light sample with its shadow ray (mis_light_part, unchanged) and one BRDF sample whose ray does both
    // jobs -- an emitter it finds is the BRDF strategy's direct estimate (Le * power weight, resolved where the ray was
    // traced), any other surface is the next vertex.  What differs from the reference's:
    //   - the BRDF sample carries the full BRDF (mis_brdf) over the mixture pdf, not the sampled lobe's;
    //   - its ray starts at the surface point h.pos, where the shadow rays start, so both MIS strategies measure a
    //     light point from one origin and their weights sum to one.  FrameConst::normal_off (rs_frame_params::
    //     normal_offset) is NOT used by this estimator; self-hits are kept off by tnear = FLT_MIN + tnear_offset;
    //   - Russian roulette (bounce > 5, q = min(max(maxc Kd, maxc Ks) of the record, 1)) is drawn after the emitter
    //     test and divides the whole return of the vertex, direct part included: its record is (Ld / q, ...);
    //   - one closest-hit ray per vertex instead of two: two walks per iteration, not three.
    // E = kEstUnbiasedSky is kEstUnbiased with the environment as a light.  A direction from a vertex
    // ends on an emitter, on another surface or in the environment; the emitters keep their two strategies, the
    // environment gets its own two, and on each domain the weights sum to one:
    //   - one sky sample per vertex (sky_light_part) when calc_di, use_skybox and the tables' total > 0, drawn after
    //     the emitter sample and before the BRDF sample; it joins Ld before sanitize and the division by q;
    //   - a BRDF ray that misses, at any vertex, the last included, brings L_env * power weight against the sky sample's
    //     density on its direction (weight 1 where there is no sky strategy: bg_color, a sky without light); nothing
    //     with calc_di off, as the emitters that ray finds count nothing then.
    // K is read by this instantiation only.
    constexpr bool U = E != kEstReference;
    constexpr bool SK = E == kEstUnbiasedSky;
    const bool sky_on = SK && F.use_sky && K.total > 0;              // the sky strategy exists (uniform)
    extern __shared__ __attribute__((aligned(16))) float path_rec[];
    constexpr int TL = T | TRAV_LANE;               // past the camera vertex every ray is incoherent
    float* const rec = path_rec + threadIdx.x;
    int x, y;
    bool in;                                                         // y: the image row -- pix, the RNG key, the store
    if constexpr (kRows) in = pixel_of_rows(F, R, x, y);
    else in = pixel_of(F, F.y0, F.y1, x, y);
    const uint64_t t0 = wave_clock();
    const uint32_t pix = (uint32_t)y * (uint32_t)F.W + (uint32_t)x;
    uint32_t rays = in ? 1u : 0u;
    vec3 dc = mk((float)x - (float)F.W / 2.0f, (float)F.H / 2.0f - (float)y, -F.cam.focal);
    const float* m = F.inv_view;
    vec3 d = normalize(mk(m[0] * dc.x + m[3] * dc.y + m[6] * dc.z, m[1] * dc.x + m[4] * dc.y + m[7] * dc.z,
                          m[2] * dc.x + m[5] * dc.y + m[8] * dc.z));
    SurfHit hi = intersect<T>(S, in, F.cam.pos, d, FLT_MIN + 0.01f);
    MatRec mr = load_mat(S, hi.mat);
    const bool surf = in && hi.hit && !any_pos(mr.le);               // Material::isEmitter: camera vertex -> Le
    vec3 px = hi.hit ? mr.le : (F.use_sky ? sky_texel(S, d) : F.bg);  // miss: sky or bgColor (:131)
    const MisSurf h0 = path_surf(S, hi, mr, d, surf);                // the camera vertex, once per pixel
    Rng rng; rng.init(F.seed, F.frame, kPassMis, pix);
    vec3 acc = mk(0, 0, 0);
    MisSurf h = h0;                                                  // the vertex this iteration handles
    int k = surf ? 0 : Q.spp, b = 0;                               // sample and bounce of that vertex
    float q = 1.0f;                                                  // its (bounce > 5 && RR) ? survival probability : 1
    // every iteration moves every live lane one vertex on and a sample has at most max_bounces + 1 of them, so
    // the bound is never what ends the loop; it is there so that nothing can spin
    const uint32_t cap = (uint32_t)Q.spp * (uint32_t)(Q.max_bounces + 1);
    for (uint32_t it = 0; it < cap; ++it) {
        const bool live = k < Q.spp;
        if (__ballot(live) == 0) break;
        vec3 Ld = mk(0, 0, 0);
        if (Q.di) {
            if constexpr (!U) {
                Ld = mk(0, 0, 0) + mis_brdf_part<TL>(S, F, h, live, rng, rays);
                Ld = Ld + mis_light_part<TL>(S, F, h, live, rng, rays);
            } else {
                Ld = mk(0, 0, 0) + mis_light_part<TL>(S, F, h, live, rng, rays);
                if constexpr (SK) {
                    if (sky_on) Ld = Ld + sky_light_part<TL>(S, F, K, h, live, rng, rays);
                }
            }
        }
        Ld = sanitize(Ld);
        if constexpr (U) Ld = dvs(Ld, q);
        vec3 R = mk(0, 0, 0);                                        // what the continuation ray brings back
        bool more = false;                                           // the path goes on at the next hit
        MisSurf hx = h;
        float qx = 1.0f;                                             // unbiased: the next vertex's q
        if (U || Q.gi) {                                             // the reference draws nothing with GI off
            vec3 f_r;
            float pdf;
            const vec3 wi = mis_sample<E>(h, rng, f_r, pdf);         // drawn even when the limit ends the path here
            bool last, go;                                           // this is the last vertex; its ray is traced
            if constexpr (!U) {
                last = b + 1 > Q.max_bounces;
                go = live && !last;                                  // (:75-76) no ray beyond the limit
            } else {
                last = !Q.gi || b + 1 > Q.max_bounces;               // the next hit counts as an emitter only,
                go = live && !(last && !Q.di);                       // which nobody asks for with the direct part off
            }
            rays += go ? 1u : 0u;
            const vec3 org = U ? h.pos : h.pos + h.n * F.normal_off; // unbiased: from where the shadow rays start
            const SurfHit nx = intersect<TL>(S, go, org, wi, FLT_MIN + F.tnear_off);
            if (live) {
                float* r = rec + b * (kPathRec * kPathBlock);
                r[0 * kPathBlock] = Ld.x; r[1 * kPathBlock] = Ld.y; r[2 * kPathBlock] = Ld.z;
                r[3 * kPathBlock] = f_r.x; r[4 * kPathBlock] = f_r.y; r[5 * kPathBlock] = f_r.z;
                r[6 * kPathBlock] = fabsf(dot(wi, h.n));
                r[7 * kPathBlock] = pdf * q;
            }
            const MatRec mx = load_mat(S, nx.mat);
            if constexpr (!SK) {
                if (go && !nx.hit && (!U || !last)) R = F.use_sky ? sky_texel(S, wi) : F.bg;
            } else if (go && !nx.hit && Q.di) {                     // the BRDF strategy's estimate of the environment
                if (sky_on) {
                    float p_sky;
                    const vec3 Le = sky_lookup(S, K, wi, p_sky);
                    R = Le * mis_power(pdf, p_sky);
                } else {
                    R = F.use_sky ? sky_texel(S, wi) : F.bg;
                }
            }
            if (go && nx.hit) {
                const float maxT = gmax(maxc(mx.kd), maxc(mx.ks));   // the record's colours, not the mapped ones
                const bool rr = b + 1 > 5 && Q.rr;
                // The reference's arm makes q the next vertex's factor in place (a second variable carried over
                // path_surf's call costs its kernels a VGPR).  That is sound only in this order: this vertex's record,
                // pdf * q, is final above, and more implies live.  The unbiased arm, whose q also divides Ld, carries
                // qx to the step below.
                bool cut = false;
                if constexpr (!U) {                                  // roulette first; the draw is made only under it
                    if (rr) cut = maxT <= rng.range(0.0f, 1.0f);
                    more = !cut && !any_pos(mx.le);                  // an emitter past the camera vertex: 0 (NEE)
                    if (more) q = rr ? maxT : 1.0f;
                } else if (any_pos(mx.le)) {                         // the BRDF strategy's direct estimate
                    float cI;
                    if (Q.di) R = mx.le * mis_emitter_w<false>(S, h.pos, h.n, pdf, nx, mx, cI);
                } else if (!last) {
                    if (rr) {
                        qx = gmin(maxT, 1.0f);
                        cut = qx <= rng.range(0.0f, 1.0f);
                    }
                    more = !cut;
                }
            }
            hx = path_surf(S, nx, mx, wi, more);
        }
        if (live && more) {
            h = hx; ++b;
            if constexpr (U) q = qx;
        }
        if (live && !more) {
            if (U || Q.gi) {
                for (int l = b; l >= 0; --l) {
                    const float* r = rec + l * (kPathRec * kPathBlock);
                    const vec3 ld = mk(r[0 * kPathBlock], r[1 * kPathBlock], r[2 * kPathBlock]);
                    const vec3 fr = mk(r[3 * kPathBlock], r[4 * kPathBlock], r[5 * kPathBlock]);
                    const vec3 li = sanitize(dvs((R * fr) * r[6 * kPathBlock], r[7 * kPathBlock]));   // (:119-126)
                    R = li + ld;                                                                      // (:129)
                }
            } else {
                R = mk(0, 0, 0) + Ld;                                // the 0 + matters for -0
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
