#include "../../oracle/restir_oracle.c"
/* TEST INFRASTRUCTURE: the checkers of rs_render_path and rs_render_path_unbiased (restir-embree_amd/csrc/rs_path.h),
 * two recursions over the oracle's own intersect / mis_* / apply_maps / mis_surf_at and one pixel driver.  Material
 * model of the MIS ground truth (Phong for PHONG/DIELECTRIC, Lambert otherwise).  RNG: pass PASS_MIS, one stream per
 * pixel, draws in the recursion's order over the samples. */
typedef struct { int32_t max_bounces, russian_roulette, calc_di, calc_gi; } or_path_params;

/* The reference's estimator: NEEPathIntegrator::integrateImpl2 (pg/NEEPathIntegrator.cpp:72-131) with
 * DirectMISIntegrator as the direct integrator, written as the recursion it is: direct plus indirect light up to
 * max_bounces, Russian roulette at bounce > 5.  calc_gi = 0 is or_render_direct_mis bit for bit
 * (tests/test_path_oracle.py). */
static v3 path_L(const fctx* F, const or_path_params* Q, hitinfo hi, v3 d, int b, rng_t* rng, uint64_t* rays) {
    const or_scene* s = F->s; const or_params* P = F->P;
    if (!hi.hit) return P->use_skybox ? sky_texel(s, d) : V(P->bg_color[0], P->bg_color[1], P->bg_color[2]);   /* :131 */
    const or_mat* m = &s->mats[s->mat[hi.prim]];
    const float maxT = gmax(maxc(m->kd), maxc(m->ks));      /* the material record's colours (:82-85) */
    const int rr = b > 5 && Q->russian_roulette;
    if (rr && maxT <= rnd(rng, 0.0f, 1.0f)) return V(0, 0, 0);                                                 /* :87-91 */
    if (nonzero_pos(m->le)) return b == 0 ? m->le : V(0, 0, 0);                                                /* :93-97 */
    const mis_surf h = mis_surf_at(s, &hi, d, m);
    v3 Ld = V(0, 0, 0);
    if (Q->calc_di) {
        Ld = add(V(0, 0, 0), mis_brdf_part(F, &h, rng, rays));
        Ld = add(Ld, mis_light_part(F, &h, rng, rays));
    }
    Ld = sanitize(Ld);
    v3 Li = V(0, 0, 0);
    if (Q->calc_gi) {
        v3 f_r; float pdf;
        v3 wi = mis_sample(&h, rng, &f_r, &pdf);            /* drawn even when the next bounce is beyond the limit */
        v3 R = V(0, 0, 0);
        if (!(b + 1 > Q->max_bounces)) {                                                                       /* :75-76 */
            hitinfo nx = intersect(F, add(h.pos, scl(h.n, P->normal_offset)), wi, FLT_MIN + P->tnear_offset, rays);
            R = path_L(F, Q, nx, wi, b + 1, rng, rays);
        }
        float c = fabsf(dot(wi, h.n));
        Li = dvs(scl(mul(R, f_r), c), pdf * (rr ? maxT : 1.0f));                                               /* :119-124 */
    }
    Li = sanitize(Li);
    return add(Li, Ld);                                                                                        /* :129 */
}

/* The unbiased estimator, and its definition: the textbook NEE + MIS path tracer.  One light sample and one BRDF
 * sample per vertex; the BRDF sample's ray both carries the path on and finds the emitters the light sample is weighed
 * against.  Differences from path_L:
 *   - the BRDF sample carries the full BRDF over the mixture pdf, not the sampled lobe's;
 *   - its ray starts at the surface point, where the shadow rays start, so both strategies measure a light point
 *     from one origin (normal_offset is not used);
 *   - Russian roulette divides the whole return of the vertex, direct part included, and is drawn after the
 *     emitter test.
 * Radiance arriving along d at the vertex hi, reached from `from` by a BRDF sample of solid-angle density ppdf. */
static v3 upath_L(const fctx* F, const or_path_params* Q, hitinfo hi, v3 d, v3 from, float ppdf, int b, int only_emit,
                  rng_t* rng, uint64_t* rays) {
    const or_scene* s = F->s; const or_params* P = F->P;
    if (!hi.hit) {
        if (only_emit) return V(0, 0, 0);
        return P->use_skybox ? sky_texel(s, d) : V(P->bg_color[0], P->bg_color[1], P->bg_color[2]);
    }
    const or_mat* m = &s->mats[s->mat[hi.prim]];
    if (nonzero_pos(m->le)) {
        if (b == 0) return m->le;
        if (!Q->calc_di) return V(0, 0, 0);
        v3 kd_, ks_; float sh_; v3 ny = hi.normal;
        apply_maps(s, hi.prim, hi.u, hi.v, s->mat[hi.prim], &kd_, &ks_, &sh_, &ny, 1);
        v3 ld = sub(hi.point, from);
        float r2 = dot(ld, ld);
        ld = nrmz(ld);
        float cY = gmax(dot(neg(ld), ny), 0.0f);
        float amf = cY / r2;
        int32_t e = s->emis_id[hi.prim];
        float pdf_light = s->area[e] / s->total_area;       /* as mis_brdf_part */
        pdf_light *= 1.0f / s->area[e];
        float w = mis_power(ppdf * amf, pdf_light);
        return scl(m->le, w);
    }
    if (only_emit) return V(0, 0, 0);
    float q = 1.0f;
    if (b > 5 && Q->russian_roulette) {
        q = gmin(gmax(maxc(m->kd), maxc(m->ks)), 1.0f);     /* the material record's colours */
        if (q <= rnd(rng, 0.0f, 1.0f)) return V(0, 0, 0);
    }
    const mis_surf h = mis_surf_at(s, &hi, d, m);
    v3 Ld = V(0, 0, 0);
    if (Q->calc_di) Ld = add(V(0, 0, 0), mis_light_part(F, &h, rng, rays));
    Ld = dvs(sanitize(Ld), q);
    v3 lobe; float pdf;
    v3 wi = mis_sample(&h, rng, &lobe, &pdf);               /* the draws, wi and the mixture pdf; always drawn */
    v3 f_r = mis_brdf(&h, wi);                              /* the full BRDF */
    if (dot(h.n, wi) < 0) f_r = V(0, 0, 0);
    const int last = !Q->calc_gi || b + 1 > Q->max_bounces;
    v3 R = V(0, 0, 0);
    if (!(last && !Q->calc_di)) {
        hitinfo nx = intersect(F, h.pos, wi, FLT_MIN + P->tnear_offset, rays);
        R = upath_L(F, Q, nx, wi, h.pos, pdf, b + 1, last, rng, rays);
    }
    float c = fabsf(dot(wi, h.n));
    v3 Li = sanitize(dvs(scl(mul(R, f_r), c), pdf * q));
    return add(Li, Ld);
}

/* one sample of a recursion at the camera vertex */
typedef v3 (*camera_fn)(const fctx*, const or_path_params*, hitinfo, v3 d, v3 eye, rng_t*, uint64_t*);
static v3 path_cam(const fctx* F, const or_path_params* Q, hitinfo hi, v3 d, v3 eye, rng_t* rng, uint64_t* rays) {
    return path_L(F, Q, hi, d, 0, rng, rays);
}
static v3 upath_cam(const fctx* F, const or_path_params* Q, hitinfo hi, v3 d, v3 eye, rng_t* rng, uint64_t* rays) {
    return upath_L(F, Q, hi, d, eye, 0.0f, 0, 0, rng, rays);
}

/* spp samples where the camera vertex is a non-emissive surface; one call, which draws nothing, for the value of a
 * miss or an emitter */
static int render_with(camera_fn L, or_ctx* c, const or_scene* s, const float* cam7, const or_params* P,
                       const or_path_params* Q, uint32_t frame_index, int spp, float* out_rgb, uint64_t* rays_out) {
    if (P->use_skybox && s->sky < 0) return -2;
    if (spp < 1 || Q->max_bounces < 0 || Q->max_bounces > 15) return -1;
    int W = c->W, H = c->H;
    or_cam cam = make_cam(cam7, W, H);
    fctx F; memset(&F, 0, sizeof F);
    F.s = s; F.c = c; F.P = P; F.frame = frame_index;
    uint64_t rc = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+:rc)
    for (int y = 0; y < H; ++y) {
        for (int x = 0; x < W; ++x) {
            size_t p = (size_t)y * W + x;
            v3 d = primary_dir(&cam, x, y, W, H);
            hitinfo hi = intersect(&F, cam.eye, d, FLT_MIN + 0.01f, &rc);
            rng_t rng = rng_init(P->seed, frame_index, PASS_MIS, (uint32_t)p);
            v3 px;
            if (hi.hit && !nonzero_pos(s->mats[s->mat[hi.prim]].le)) {
                v3 acc = V(0, 0, 0);
                for (int k = 0; k < spp; ++k) acc = add(acc, L(&F, Q, hi, d, cam.eye, &rng, &rc));
                px = dvs(acc, (float)spp);
            } else {
                px = L(&F, Q, hi, d, cam.eye, &rng, &rc);
            }
            px = sanitize(px);
            out_rgb[3 * p] = px.x; out_rgb[3 * p + 1] = px.y; out_rgb[3 * p + 2] = px.z;
        }
    }
    if (rays_out) *rays_out = rc;
    return 0;
}

int or_render_path(or_ctx* c, const or_scene* s, const float* cam7, const or_params* P, const or_path_params* Q,
                   uint32_t frame_index, int spp, float* out_rgb, uint64_t* rays_out) {
    return render_with(path_cam, c, s, cam7, P, Q, frame_index, spp, out_rgb, rays_out);
}
int or_render_path_unbiased(or_ctx* c, const or_scene* s, const float* cam7, const or_params* P, const or_path_params* Q,
                            uint32_t frame_index, int spp, float* out_rgb, uint64_t* rays_out) {
    return render_with(upath_cam, c, s, cam7, P, Q, frame_index, spp, out_rgb, rays_out);
}
