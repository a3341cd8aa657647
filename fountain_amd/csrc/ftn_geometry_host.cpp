/*
 * ftn_geometry_host.cpp -- the transform, sphere, camera and film part of the C ABI (include/fountain_hip.h): exact f32 restatements of the
 * reference's host-only constructors -- Transform algebra (src/geometry/transform.rs), Sphere::new, PerspectiveCamera::new, Film::new /
 * sample_bounds / tiles.  Pure host code: nothing here needs a device, and nothing here decides what a kernel reads.
 */
#include "ftn_host_internal.h"

#include <cstring>

using namespace ftn;

/* ================================================================== Transform algebra (cgmath 0.17 Matrix4 semantics) */
static void m4_identity(float* m) { for (int i = 0; i < 16; i++) m[i] = (i % 5 == 0) ? 1.0f : 0.0f; }
static void m4_mul(const float* l, const float* r, float* o) {   /* column j = l0*r[j][0] + l1*r[j][1] + l2*r[j][2] + l3*r[j][3] */
    float t[16];
    for (int j = 0; j < 4; j++) for (int i = 0; i < 4; i++)
        t[j * 4 + i] = ((l[i] * r[j * 4] + l[4 + i] * r[j * 4 + 1]) + l[8 + i] * r[j * 4 + 2]) + l[12 + i] * r[j * 4 + 3];
    memcpy(o, t, sizeof(t));
}
/* cgmath det_sub_proc_unsafe(m, x, y, z) */
static void m4_det_sub(const float* s, int x, int y, int z, float out[4]) {
    const float a[4] = {s[4 + x], s[12 + x], s[x], s[8 + x]}, b[4] = {s[8 + y], s[8 + y], s[4 + y], s[4 + y]}, c[4] = {s[12 + z], s[z], s[12 + z], s[z]};
    const float d[4] = {s[8 + x], s[8 + x], s[4 + x], s[4 + x]}, e[4] = {s[12 + y], s[y], s[12 + y], s[y]}, f[4] = {s[4 + z], s[12 + z], s[z], s[8 + z]};
    const float g[4] = {s[12 + x], s[x], s[12 + x], s[x]}, h[4] = {s[4 + y], s[12 + y], s[y], s[8 + y]}, i[4] = {s[8 + z], s[8 + z], s[4 + z], s[4 + z]};
    for (int k = 0; k < 4; k++) {
        float t = a[k] * (b[k] * c[k]);
        t += d[k] * (e[k] * f[k]); t += g[k] * (h[k] * i[k]);
        t -= a[k] * (e[k] * i[k]); t -= d[k] * (h[k] * c[k]); t -= g[k] * (b[k] * f[k]);
        out[k] = t;
    }
}
static float m4_det(const float* m) { float t[4]; m4_det_sub(m, 1, 2, 3, t); return ((t[0] * m[0] + t[1] * m[4]) + t[2] * m[8]) + t[3] * m[12]; }
static bool m4_invert(const float* m, float* o) {
    float t0[4], t1[4], t2[4], t3[4];
    m4_det_sub(m, 1, 2, 3, t0);
    float det = ((t0[0] * m[0] + t0[1] * m[4]) + t0[2] * m[8]) + t0[3] * m[12];
    if (det == 0.0f) return false;
    float inv_det = 1.0f / det;
    m4_det_sub(m, 0, 3, 2, t1); m4_det_sub(m, 0, 1, 3, t2); m4_det_sub(m, 0, 2, 1, t3);
    for (int k = 0; k < 4; k++) { o[k] = t0[k] * inv_det; o[4 + k] = t1[k] * inv_det; o[8 + k] = t2[k] * inv_det; o[12 + k] = t3[k] * inv_det; }
    return true;
}
static void tf_mul(const ftn_transform* a, const ftn_transform* b, ftn_transform* o) {   /* transform.rs:143-149 */
    ftn_transform r; m4_mul(a->m, b->m, r.m); m4_mul(b->inv, a->inv, r.inv); *o = r;
}

extern "C" {

int ftn_transform_identity(ftn_transform* out) { m4_identity(out->m); m4_identity(out->inv); return FTN_OK; }
int ftn_transform_translate(const float d[3], ftn_transform* out) {              /* :62-66 */
    m4_identity(out->m); m4_identity(out->inv);
    for (int i = 0; i < 3; i++) { out->m[12 + i] = d[i]; out->inv[12 + i] = -d[i]; }
    return FTN_OK;
}
int ftn_transform_scale(float sx, float sy, float sz, ftn_transform* out) {      /* :68-72 */
    m4_identity(out->m); m4_identity(out->inv);
    out->m[0] = sx; out->m[5] = sy; out->m[10] = sz;
    out->inv[0] = 1.0f / sx; out->inv[5] = 1.0f / sy; out->inv[10] = 1.0f / sz;
    return FTN_OK;
}
int ftn_transform_from_flat(const float m[16], ftn_transform* out) {             /* :23-39 */
    ftn_transform r; memcpy(r.m, m, 64);
    if (!m4_invert(r.m, r.inv)) return fail(FTN_ERR_INVALID_ARGUMENT, "Could not invert matrix");
    *out = r; return FTN_OK;
}
int ftn_transform_rotate(float angle_deg, const float axis[3], ftn_transform* out) {   /* :74-78; Matrix4::from_axis_angle */
    V3 a = normalize(V3(axis[0], axis[1], axis[2]));
    float ang = angle_deg * (float)(3.14159265358979323846 / 180.0);             /* Rad::from(Deg) */
    float s = ftn_det::sinf_det(ang), c = ftn_det::cosf_det(ang), omc = 1.0f - c;
    float f[16] = {omc * a.x * a.x + c,       omc * a.x * a.y + s * a.z, omc * a.x * a.z - s * a.y, 0.0f,
                   omc * a.x * a.y - s * a.z, omc * a.y * a.y + c,       omc * a.y * a.z + s * a.x, 0.0f,
                   omc * a.x * a.z + s * a.y, omc * a.y * a.z - s * a.x, omc * a.z * a.z + c,       0.0f,
                   0.0f, 0.0f, 0.0f, 1.0f};
    return ftn_transform_from_flat(f, out);
}
int ftn_transform_look_at(const float p[3], const float l[3], const float u[3], ftn_transform* out) {   /* :41-56 */
    V3 pos(p[0], p[1], p[2]);
    V3 dir = normalize(V3(l[0], l[1], l[2]) - pos);
    V3 right = normalize(cross(normalize(V3(u[0], u[1], u[2])), dir));
    V3 new_up = cross(dir, right);
    float mat[16] = {right.x, right.y, right.z, 0.0f, new_up.x, new_up.y, new_up.z, 0.0f, dir.x, dir.y, dir.z, 0.0f, pos.x, pos.y, pos.z, 1.0f};
    ftn_transform r; memcpy(r.inv, mat, 64);
    if (!m4_invert(mat, r.m)) return fail(FTN_ERR_INVALID_ARGUMENT, "Could not invert matrix");
    *out = r; return FTN_OK;
}
int ftn_transform_mul(const ftn_transform* a, const ftn_transform* b, ftn_transform* out) { tf_mul(a, b, out); return FTN_OK; }
int ftn_transform_inverse(const ftn_transform* a, ftn_transform* out) { ftn_transform r; memcpy(r.m, a->inv, 64); memcpy(r.inv, a->m, 64); *out = r; return FTN_OK; }
int ftn_transform_perspective(float fov, float n, float f, ftn_transform* out) {   /* :105-115 */
    float m[16] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, f / (f - n), 1.0f, 0.0f, 0.0f, -f * n / (f - n), 0.0f};
    float inv_tan_ang = 1.0f / ftn_det::tanf_det((fov * (FTN_PI / 180.0f)) / 2.0f);   /* f32::to_radians */
    ftn_transform p, s;
    int rc = ftn_transform_from_flat(m, &p); if (rc) return rc;
    ftn_transform_scale(inv_tan_ang, inv_tan_ang, 1.0f, &s);
    tf_mul(&s, &p, out);
    return FTN_OK;
}
int ftn_transform_point(const ftn_transform* t, const float p[3], float o[3]) { V3 r = m4_point(t->m, V3(p[0], p[1], p[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; return FTN_OK; }
int ftn_transform_vector(const ftn_transform* t, const float p[3], float o[3]) { V3 r = m4_vector(t->m, V3(p[0], p[1], p[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; return FTN_OK; }
int ftn_transform_normal(const ftn_transform* t, const float p[3], float o[3]) { V3 r = m4_normal(t->inv, V3(p[0], p[1], p[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; return FTN_OK; }
int ftn_transform_swaps_handedness(const ftn_transform* t) { return m4_det(t->m) < 0.0f ? 1 : 0; }
int ftn_transform_points(const ftn_transform* t, size_t n, const float* in, float* out) {
    for (size_t i = 0; i < n; i++) { V3 r = m4_point(t->m, V3(in[3 * i], in[3 * i + 1], in[3 * i + 2])); out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z; }
    return FTN_OK;
}
int ftn_transform_normals(const ftn_transform* t, size_t n, const float* in, float* out) {
    for (size_t i = 0; i < n; i++) { V3 r = m4_normal(t->inv, V3(in[3 * i], in[3 * i + 1], in[3 * i + 2])); out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z; }
    return FTN_OK;
}

/* ================================================================== Sphere::new / PerspectiveCamera::new / Film */
int ftn_sphere_init(const ftn_transform* o2w, const ftn_transform* w2o, int rev, float radius, float z_min, float z_max, float phi_max_deg, ftn_sphere* out) {
    memset(out, 0, sizeof(*out));                                                 /* sphere.rs:30-50 */
    out->object_to_world = *o2w; out->world_to_object = *w2o; out->reverse_orientation = rev ? 1u : 0u;
    out->radius = radius;
    out->z_min = clampf(fmin_(z_min, z_max), -radius, radius);
    out->z_max = clampf(fmax_(z_min, z_max), -radius, radius);
    out->theta_min = ftn_det::acosf_det(clampf(z_min / radius, -1.0f, 1.0f));
    out->theta_max = ftn_det::acosf_det(clampf(z_max / radius, -1.0f, 1.0f));
    out->phi_max = clampf(phi_max_deg, 0.0f, 360.0f) * (FTN_PI / 180.0f);
    return FTN_OK;
}
int ftn_camera_perspective(const ftn_transform* c2w, const int32_t res[2], const float sw[4], const float sh[2], float lens_radius, float focal_dist,
                           float fov, ftn_camera_desc* out) {                   /* camera/mod.rs:51-69, 85-114 */
    memset(out, 0, sizeof(*out));
    ftn_transform persp, s1, s2, tr, s2r, s2r_inv, pinv, r2c;
    int rc = ftn_transform_perspective(fov, 1.0e-2f, 1000.0f, &persp); if (rc) return rc;
    ftn_transform_scale((float)res[0], (float)res[1], 1.0f, &s1);
    ftn_transform_scale(1.0f / (sw[2] - sw[0]), 1.0f / (sw[1] - sw[3]), 1.0f, &s2);
    const float d[3] = {-sw[0], -sw[3], 0.0f};
    ftn_transform_translate(d, &tr);
    ftn_transform t12; tf_mul(&s1, &s2, &t12); tf_mul(&t12, &tr, &s2r);           /* screen_to_raster */
    ftn_transform_inverse(&s2r, &s2r_inv);                                       /* raster_to_screen */
    ftn_transform_inverse(&persp, &pinv);
    tf_mul(&pinv, &s2r_inv, &r2c);                                               /* raster_to_camera */
    out->camera_to_world = *c2w; out->raster_to_camera = r2c;
    out->shutter_open = sh[0]; out->shutter_close = sh[1]; out->lens_radius = lens_radius; out->focal_dist = focal_dist;
    V3 o = m4_point(r2c.m, V3(0.0f, 0.0f, 0.0f));
    V3 dx = m4_point(r2c.m, V3(1.0f, 0.0f, 0.0f)) - o, dy = m4_point(r2c.m, V3(0.0f, 1.0f, 0.0f)) - o;
    out->dx_camera[0] = dx.x; out->dx_camera[1] = dx.y; out->dx_camera[2] = dx.z;
    out->dy_camera[0] = dy.x; out->dy_camera[1] = dy.y; out->dy_camera[2] = dy.z;
    return FTN_OK;
}
int ftn_film_init(const int32_t res[2], const float cw[4], ftn_film_desc* out) {   /* film.rs:43-58 */
    out->full_resolution[0] = res[0]; out->full_resolution[1] = res[1];
    out->crop[0] = f2i_sat(ceilf((float)res[0] * cw[0])); out->crop[1] = f2i_sat(ceilf((float)res[1] * cw[1]));
    out->crop[2] = f2i_sat(ceilf((float)res[0] * cw[2])); out->crop[3] = f2i_sat(ceilf((float)res[1] * cw[3]));
    out->filter_radius[0] = 0.5f; out->filter_radius[1] = 0.5f;
    return FTN_OK;
}
int ftn_film_sample_bounds(const ftn_film_desc* f, int32_t o[4]) {                 /* film.rs:86-93 */
    o[0] = f2i_sat(floorf((float)f->crop[0] + 0.5f - f->filter_radius[0])); o[1] = f2i_sat(floorf((float)f->crop[1] + 0.5f - f->filter_radius[1]));
    o[2] = f2i_sat(ceilf((float)f->crop[2] - 0.5f + f->filter_radius[0])); o[3] = f2i_sat(ceilf((float)f->crop[3] - 0.5f + f->filter_radius[1]));
    return FTN_OK;
}
int ftn_film_tile_count(const ftn_film_desc* f, uint32_t* out) { std::vector<DTile> t; list_tiles(f, &t); *out = (uint32_t)t.size(); return FTN_OK; }
int ftn_film_resolve(const ftn_pixel* p, size_t n, float* rgb_out) {               /* film.rs:195-210 (host buffers; output stage) */
    for (size_t i = 0; i < n; i++) {
        float rgb[3]; xyz_to_rgb(p[i].xyz, rgb);
        if (p[i].filter_weight_sum != 0.0f) { float inv = 1.0f / p[i].filter_weight_sum; for (int c = 0; c < 3; c++) rgb[c] = fmax_(0.0f, rgb[c] * inv); }
        rgb_out[3 * i] = rgb[0]; rgb_out[3 * i + 1] = rgb[1]; rgb_out[3 * i + 2] = rgb[2];
    }
    return FTN_OK;
}

}  /* extern "C" */

void list_tiles(const ftn_film_desc* f, std::vector<DTile>* tiles) {               /* bounds.rs:85-97, integrator/mod.rs:182-185 */
    int32_t sb[4]; ftn_film_sample_bounds(f, sb);
    for (int y = sb[1]; y < sb[3]; y += 16) for (int x = sb[0]; x < sb[2]; x += 16) {
        DTile t; t.valid_off = 0; t._pad = 0; t.x0 = x; t.y0 = y; t.x1 = std::min(x + 16, sb[2]); t.y1 = std::min(y + 16, sb[3]);
        t.tile_id = (unsigned long long)(long long)(t.y0 * sb[2] + t.x0);
        tiles->push_back(t);
    }
}
