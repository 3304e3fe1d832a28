// rs_mis.h -- MIS direct-light ground truth: converged references for bias/variance
// checks of the ReSTIR output.
//
// SimpleGuiDX11::produceStandard (pg/simpleguidx11.cpp:336-357) with Raytracer::get_pixel
// (pg/raytracer.cpp:40-45) and NEEPathIntegrator::integrateImpl2 (pg/NEEPathIntegrator.cpp:72-131) at
// calcDI = on, calcGI = off (direct illumination: the quantity ReSTIR DI estimates), with
// DirectMISIntegrator as the direct integrator (pg/DirectMISIntegrator.cpp:10-143): per sample one
// BRDF-sampled ray, then one light sample with its shadow ray, power heuristic.  Material calls are the
// HitInfo variants: MaterialLambert (pg/MaterialLambert.cpp:10-31), MaterialPhong
// (pg/MaterialPhong.cpp:18-119); Phong for PHONG/DIELECTRIC, Lambert for the other types (the ReSTIR
// path's BRDF model, pg/ReSTIRIntegrator.h:32-41, so both converge to the same image).  Pixel-corner
// primary ray (CenterSampler), computed once per pixel; spp samples per launch averaged (sum / spp);
// frames are accumulated by rs_post_frame (the reference's running mean).  RNG: pass kPassMis, draws
// sequential per pixel over the samples.  Restated in oracle/restir_oracle.c or_render_direct_mis.
#pragma once
#include "rs_passes.h"

namespace rs {

constexpr uint32_t kPassMis = 64u;
// the estimators of the ground truths: the reference's, restated bit for bit with its three biases, and
// the textbook NEE + MIS one over the same material model (rs_path.h)
// kEstUnbiasedSky: the unbiased one with the environment as a light (rs_path.h, rs_sky.h)
constexpr int kEstReference = 0, kEstUnbiased = 1, kEstUnbiasedSky = 2;

struct MisSurf { vec3 pos, n, wr, kd, ks; float shin, i_m, maxD, maxS, pf; bool phong; };

// The rows of a ground-truth launch (rs_row_set): image rows y with (y / strip_rows) % stride == phase, strip_rows a
// multiple of the workgroup tile's 16 rows.  The launch covers them packed as virtual rows v = 0, 1, ...: a
// workgroup's 16 virtual rows lie in one strip, so the strip and the image row of its first virtual row are
// wave-uniform (scalar registers, computed once); {16, 1, 0} is every row at its place, the full frame.
struct RowSet { int strip_rows, stride, phase; };

// pixel_of over a row set: whether the pixel exists; x / y clamped into the image as pixel_of clamps them
__device__ __forceinline__ bool pixel_of_rows(const FrameConst& F, const RowSet& R, int& x, int& y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int v0 = (int)blockIdx.y * 16;                              // the workgroup's first virtual row
    const int s = v0 / R.strip_rows;                                  // its strip among the set's own
    const int y0 = (s * R.stride + R.phase) * R.strip_rows + (v0 - s * R.strip_rows);
    x = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    y = y0 + (wave >> 1) * 8 + (lane >> 3);
    const bool in = x < F.W && y < F.H;
    x = x < F.W ? x : F.W - 1;
    y = y < F.H ? y : F.H - 1;
    return in;
}

// DirectMISIntegrator::powerHeuristic (pg/DirectMISIntegrator.cpp:10-15)
__device__ __forceinline__ float mis_power(float pdf, float other) {
    float a = pdf * pdf, b = other * other;
    return a / (b + a);
}
__device__ __forceinline__ vec3 dvs(vec3 v, float s) { return mk(v.x / s, v.y / s, v.z / s); }   // glm vec3 / scalar
__device__ __forceinline__ float cos_pdf(vec3 n, vec3 wi) { return gmax(dot(n, wi), 0.0f) * kOneOverPi; }
// The lobe's power on wi for the pdf (base max(0, d)) and for the BRDF (base max(d, 0)), as rs_device.h lobe_pow:
// one pow where the two bases are the same bits, the BRDF's own only where they are not (d NaN or -0: no core)
__device__ __forceinline__ LobePow mis_lobe_pow(const MisSurf& h, vec3 wi) {
    LobePow r{0.0f, 0.0f};
    if (!h.phong) return r;
    const float bp = gmax(0.0f, dot(wi, h.wr)), bb = gmax(dot(wi, h.wr), 0.0f);
    r.pdf = r.brdf = rs_powf(bp, h.shin);
    const bool own = __float_as_uint(bp) != __float_as_uint(bb);
    if (__ballot(own) != 0) {
        if (own) r.brdf = rs_powf_sel(bb, h.shin, RS_LM_POW_EDGE);
    }
    return r;
}
__device__ __forceinline__ float lobe_pdf(float g, float pw) {              // pg/Distribution.h:65-67
    return (g + 1.0f) * kOneOver2Pi * pw;
}
// getPdfForSample (pg/MaterialLambert.cpp:20-23, pg/MaterialPhong.cpp:94-119)
__device__ __forceinline__ float mis_pdf_for(const MisSurf& h, vec3 wi, const LobePow& lp) {
    if (!h.phong) return cos_pdf(h.n, wi);
    float pdf = cos_pdf(h.n, wi) * h.pf;
    pdf += lobe_pdf(h.shin, lp.pdf) * (1.0f - h.pf);
    return pdf;
}
// evaluateBRDF (pg/MaterialLambert.cpp:25-31, pg/MaterialPhong.cpp:69-92)
__device__ __forceinline__ vec3 mis_brdf(const MisSurf& h, const LobePow& lp) {
    vec3 f = h.kd * kOneOverPi;
    if (!h.phong) return f;
    return f + (h.ks * h.i_m) * lp.brdf;
}
// evaluateLightingGI (pg/MaterialLambert.cpp:10-18, pg/MaterialPhong.cpp:18-67): the lobe choice, wi, one power for
// the pdf and the BRDF, the mixture pdf, f_r zeroed below the surface.  f_r is the estimator's own.  The reference's is
// the sampled lobe's, and its Lambert returns early with kd / pi, never zeroed; the unbiased one's is the full BRDF on
// wi (kd * (1 / pi) + ...: other bits).  Past the Lambert return the reference's form has h.phong true; the conditions
// spell that out (E == kEstReference ||) so that its kernels compile to the text they had before the two forms met.
template <int E>
__device__ __forceinline__ vec3 mis_sample(const MisSurf& h, Rng& rng, vec3& f_r, float& pdf) {
    if (E == kEstReference && !h.phong) {
        vec3 wi = cosine_sample(h.n, rng);
        pdf = cos_pdf(h.n, wi);
        f_r = dvs(h.kd, kPi);
        return wi;
    }
    bool diffuse = true;
    if (E == kEstReference || h.phong) diffuse = rng.range(0.0f, h.maxD + h.maxS) < h.maxD;
    vec3 wi;
    if (diffuse) wi = cosine_sample(h.n, rng);
    else wi = lobe_sample(h.wr, h.shin, rng);
    const LobePow lp = mis_lobe_pow(h, wi);
    if constexpr (E != kEstReference) {
        pdf = mis_pdf_for(h, wi, lp);
        f_r = mis_brdf(h, lp);
    } else {
        if (diffuse) f_r = h.kd * kOneOverPi;
        else f_r = (h.ks * h.i_m) * lp.brdf;
        float pd = cos_pdf(h.n, wi) * h.pf;
        float ps = lobe_pdf(h.shin, lp.pdf) * (1.0f - h.pf);
        pdf = pd + ps;
    }
    if (dot(h.n, wi) < 0) f_r = mk(0, 0, 0);
    return wi;
}

// The BRDF ray from `from`, drawn with solid-angle pdf `pdf`, hit the emitter b of material record m: the power
// heuristic's weight of that strategy (pg/DirectMISIntegrator.cpp:118-140); kCosI: cI becomes the cosine at `from`, normal n,
// in the place the operation had in mis_brdf_part; the unbiased vertex does not want it and its cI stays untouched
template <bool kCosI>
__device__ __forceinline__ float mis_emitter_w(const DevScene& S, vec3 from, vec3 n, float pdf, const SurfHit& b, MatRec m,
                                               float& cI) {
    vec3 bn = b.normal;
    if (S.texd) apply_maps(S, b, m, bn, true);
    vec3 ld = b.point - from;
    float r2 = dot(ld, ld);
    ld = normalize(ld);
    if constexpr (kCosI) cI = gmax(dot(ld, n), 0.0f);
    float cY = gmax(dot(-ld, bn), 0.0f);
    float amf = cY / r2;
    return mis_power(pdf * amf, emis_pdf_brdf(S, b.emis_id));     // TriangleCDF::getPDFForTriangle
}

// DirectMISIntegrator::evaluateBRDFSample (pg/DirectMISIntegrator.cpp:94-144).  BRDF rays are
// incoherent: per-lane walk (as brdf_sample in the ReSTIR passes).
template <int T>
__device__ __forceinline__ vec3 mis_brdf_part(const DevScene& S, const FrameConst& F, const MisSurf& h, bool alive,
                                              Rng& rng, uint32_t& rays) {
    vec3 f_r;
    float pdf;
    vec3 wi = mis_sample<kEstReference>(h, rng, f_r, pdf);
    rays += alive ? 1u : 0u;
    SurfHit b = intersect<T | TRAV_LANE>(S, alive, h.pos + h.n * F.normal_off, wi, FLT_MIN + F.tnear_off);
    if (!b.hit) return mk(0, 0, 0);
    MatRec m = load_mat(S, b.mat);
    if (!(m.le.x + m.le.y + m.le.z > 0)) return mk(0, 0, 0);      // Material::isEmissive
    float cI;
    float w = mis_emitter_w<true>(S, h.pos, h.n, pdf, b, m, cI);
    return dvs(((m.le * w) * f_r) * cI, pdf);
}

// DirectMISIntegrator::evaluateLightSample (pg/DirectMISIntegrator.cpp:38-92)
template <int T>
__device__ __forceinline__ vec3 mis_light_part(const DevScene& S, const FrameConst& F, const MisSurf& h, bool alive,
                                               Rng& rng, uint32_t& rays) {
    if (S.n_emis == 0) return mk(0, 0, 0);                          // TriangleCDF::isValid (uniform)
    float ksi = rng.range(0.0f, 1.0f);                              // TriangleCDF::getTriangle
    const uint32_t idx = light_index(S, ksi);
    const EmisRec E = EmisRec::load(S.emis + 8 * idx);
    float r1 = rng.range(0, 1), r2 = rng.range(0, 1);                // Sampling::sampleTriangle
    float sr = sqrtf(r1);
    float bx = 1.0f - sr, by = sr * (1.0f - r2), bz = sr * r2;
    vec3 pt = (E.p0 * bx + E.p1 * by) + E.p2 * bz;
    vec3 nn = normalize((E.n0 * bx + E.n1 * by) + E.n2 * bz);
    float light_pdf = E.pdf_area;                                    // pick prob * (1 / area)
    vec3 ld = pt - h.pos;
    float r_sqr = dot(ld, ld);
    ld = normalize(ld);
    float cI = gmax(dot(ld, h.n), 0.0f);
    float cY = gmax(dot(-ld, nn), 0.0f);
    float amf = cY / r_sqr;
    const bool ok = alive && light_pdf != 0.0f && r_sqr != 0.0f && cI > 0 && cY > 0;
    const bool occ = occluded<T>(S, F, ok, h.pos, pt, rays);
    if (!ok || occ) return mk(0, 0, 0);
    const LobePow lp = mis_lobe_pow(h, ld);
    float pba = mis_pdf_for(h, ld, lp) * amf;
    float w = mis_power(light_pdf, pba);
    if (!(w > 0.0f)) return mk(0, 0, 0);
    float G = cI * cY / r_sqr;
    return dvs(((E.le * w) * mis_brdf(h, lp)) * G, light_pdf);
}

// kRows: the launch covers the row set R (rs_render_ground_truth_rows); else rows [F.y0, F.y1) and R is not read --
// the full-frame entries keep the instantiation they had (through the row-set form the reference's
// path tracer measured 0.8-1.1 % slower at equal registers)
template <int T, bool kRows = false>
__global__ void __launch_bounds__(256) k_direct_mis(DevScene S, FrameConst F, int spp, float* fb, CountSlot C,
                                                        RowSet R) {
    int x, y;
    bool in;
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
    vec3 hn = hi.normal;
    if (S.texd && hi.hit) apply_maps(S, hi, mr, hn, false);
    const bool surf = in && hi.hit && !any_pos(mr.le);               // Material::isEmitter: camera vertex -> Le
    vec3 px = hi.hit ? mr.le : (F.use_sky ? sky_texel(S, d) : F.bg);  // miss: sky or bgColor (:131)
    MisSurf h;
    h.pos = hi.point; h.n = hn; h.kd = mr.kd; h.ks = mr.ks; h.shin = mr.shin;
    h.phong = is_phong(mr.type);
    h.maxD = maxc(h.kd); h.maxS = maxc(h.ks);
    h.pf = h.maxD / (h.maxD + h.maxS);
    h.wr = normalize(reflect(d, h.n));
    h.i_m = (surf && h.phong) ? 1.0f / calc_I_M(dot(-d, h.n), h.shin) : 0.0f;
    Rng rng; rng.init(F.seed, F.frame, kPassMis, pix);
    vec3 acc = mk(0, 0, 0);
    for (int k = 0; k < spp; ++k) {
        vec3 L = mk(0, 0, 0) + mis_brdf_part<T>(S, F, h, surf, rng, rays);
        L = L + mis_light_part<T>(S, F, h, surf, rng, rays);
        acc = acc + (mk(0, 0, 0) + sanitize(L));                    // L_i_indirect (0) + L_i_direct
    }
    if (surf) px = dvs(acc, (float)spp);
    px = sanitize(px);
    if (in) store_rgb(fb, pix, px);
    count_rays(C, rays, in ? 1u : 0u, t0, y);
}

}  // namespace rs
