/*
 * humanoid_render.h -- C ABI of libhumanoid_render.so, the headless camera sensors of the MI355X
 * (gfx950) humanoid engine: one HIP ray-casting kernel that draws the engine's analytic scene (24
 * sphere / capsule / box geoms per env on a ground plane) straight from the rigid-body state buffer
 * that is already on the device. It replaces the camera-sensor half of Isaac Gym's graphics API as
 * puffer_phc/envs/render_env.py uses it (create_camera_sensor :218-227, set_camera_location
 * :398-411, render_all_camera_sensors + get_camera_image :151-171, the red marker spheres of the
 * reference motion :306-335, :416-450). There is no window: the GPU machines are headless.
 *
 * The library is separate from libhumanoid_engine.so and only READS the engine's buffers through
 * device pointers: nothing here is linked into the engine, whose device code stays as it is.
 *
 * Conventions (those of humanoid_engine.h)
 *   - every entry point returns 0 on success, non-zero on failure; hr_last_error() gives the text;
 *   - float / int pointers passed to hr_set_appearance, hr_set_markers (pos) and hr_render are DEVICE
 *     pointers on the handle's device, owned by the caller; `stream` is a hipStream_t (NULL = default
 *     stream); hr_render does not synchronise the host. hr_set_cameras and hr_set_markers upload a few
 *     bytes with a blocking copy (setup calls, ordered after work on the default stream);
 *   - quaternions are xyzw, Z-up; rows of rb_state are pos3 quat4 linvel3 angvel3 (HE_BUF_RB_STATE).
 *
 * ---------------------------------------------------------------------------------------------
 * THE IMAGE (the definition a test restates; all arithmetic is float32 on the device)
 *
 * rot(q, v) for a unit quaternion q = (x, y, z, w) = (qv, w):  t = 2 (qv x v);  rot = (v + w t) + qv x t.
 * A cross product a x b has components (ay bz - az by, az bx - ax bz, ax by - ay bx).
 *
 * Camera. A fixed camera (follow_body = -1) has the world points P = pos, T = target. A following
 * camera reads row (env * 24 + follow_body) of rb_state at render time (body position p, rotation q):
 * mode 0 (position):  P = p + pos,  T = p + target;  mode 1 (transform):  P = p + rot(q, pos),
 * T = p + rot(q, target);  mode 2 (position xy): as mode 0 in x and y, while P_z = pos_z and
 * T_z = target_z stay absolute heights (a tracking shot that does not bob with the body). These few
 * operations are evaluated exactly as written, each product and sum rounded to float32 on its own (no
 * fused multiply-add), so a fixed camera placed at a P and T computed the same way on the host draws
 * the same image bit for bit.
 *   f = normalize(T - P);  r = normalize(f x (0,0,1)), and when |f x (0,0,1)| < 1e-6, r =
 *   normalize(f x (0,1,0));  u = r x f.
 * Pixel (row i, column j) of a W x H image, with th = tan(hfov / 2):
 *   x = (2 (j + 1/2) / W - 1) th;   y = (1 - 2 (i + 1/2) / H) th H / W;   d = normalize(f + x r + y u).
 * The ray is o + t d with o = P.
 *
 * Scene of a camera: the 24 geoms of ITS OWN env only (the envs share one world frame with a sub-metre
 * xy jitter; drawing all of them would pile them up), that env's markers, and the plane z = 0. The
 * terrain kinds 1 and 2 of the engine's per-env terrain option (slope, steps) are drawn as the flat
 * plane. Body b (row p, q of rb_state) carries one geom, given in the body frame by the model:
 *   sphere   geom_params = (c3, r):            centre C = p + rot(q, c), radius r;
 *   capsule  geom_params = (a3, b3, r):        A = p + rot(q, a), B = p + rot(q, b), L = |B - A|,
 *                                              axis w = (B - A) / L (L < 1e-9: w = (0,0,1), L = 0);
 *   box      geom_params = (c3, e3, qb4):      centre C = p + rot(q, c), half extents e, rotation
 *                                              matrix R of the Hamilton product q * qb (columns = the
 *                                              box axes in the world; the usual unit-quaternion matrix
 *                                              1 - 2(y^2 + z^2), 2(xy - wz), ... ).
 * A marker k is a sphere of the common marker radius at the world point pos[env][k].
 *
 * Hits. Only ENTRY hits count: a ray that starts inside a primitive does not hit it.
 *   sphere (C, r):   m = o - C;  b = m.d;  q = m - b d;  h = r^2 - q.q;  hit when h >= 0 at
 *                    t = -b - sqrt(h), normal (m + t d) / r.  (h is formed from the perpendicular
 *                    offset, so a grazing ray does not cancel.)
 *   capsule:         the nearest of: the two cap spheres (A, r), (B, r), and the cylinder: m = o - A,
 *                    mp = m - (m.w) w,  dp = d - (d.w) w,  a = dp.dp,  c = mp x dp,
 *                    h = a r^2 - c.c;  when a >= 1e-12 and h >= 0:  t = (-(mp.dp) - sqrt(h)) / a,
 *                    s = m.w + t (d.w), a hit when 0 <= s <= L with normal (mp + t dp) / r.
 *   box:             ol = R^T (o - C), dl = R^T d;  per axis k: t1 = (-e_k - ol_k) / dl_k,
 *                    t2 = (e_k - ol_k) / dl_k, lo_k = min(t1, t2), hi_k = max(t1, t2) (IEEE division;
 *                    an axis with dl_k = 0 gives -inf / +inf when ol_k is inside the slab, and no hit
 *                    when outside);  tn = max lo_k, tf = min hi_k;  a hit when tn <= tf at t = tn.
 *                    The normal is -sign(dl_k) R[:,k] for the first axis k (x, y, z) with lo_k = tn.
 *   ground:          when d_z < 0 and o_z > 0:  t = -o_z / d_z, normal (0,0,1).
 * A hit is kept when near <= t <= far. The nearest kept hit wins; candidates are visited in the order
 * ground, bodies 0..23, markers 0..m-1, and a later one replaces the current one only when its t is
 * strictly smaller.
 *
 * Outputs per pixel
 *   depth  -t (d.f): negative view-space distance, as Isaac Gym documents its depth image; -inf where
 *          nothing is hit. (Neither PhysX nor the Isaac renderer is available to pin this against.)
 *   seg    the body's segmentation id, HR_SEG_MARKER for a marker, 0 for ground and sky.
 *   colour sky: HR_SKY_*. Otherwise albedo (HR_AMBIENT + (1 - HR_AMBIENT) max(0, n.l) s) per channel,
 *          with the unit light direction l = (HR_LIGHT_X, HR_LIGHT_Y, HR_LIGHT_Z) (towards the
 *          light). s = HR_SHADOW when shadows are on, n.l > 0 and the shadow ray
 *          (o' = hit point + HR_SHADOW_EPS n, direction l) has an entry hit with t >= 0 on ANY of
 *          the 24 body geoms of the env (markers cast no shadow); otherwise s = 1.
 *          albedo: the body's colour; the marker's colour; the ground: with the checker on,
 *          HR_GROUND_EVEN when floor(x) + floor(y) of the hit point (o + t d) is even, HR_GROUND_ODD
 *          when odd (a grey, the same in all three channels); with it off, HR_GROUND_EVEN.
 *          Each channel c is clamped to [0, 1] and stored as (int)(c 255 + 0.5); alpha is 255.
 *          A pixel is 4 bytes R, G, B, A.
 */
#ifndef HUMANOID_RENDER_H
#define HUMANOID_RENDER_H

#include <stdint.h>

#include "humanoid_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* image constants (restated in DESIGN.md) */
#define HR_AMBIENT 0.35f
#define HR_SHADOW 0.4f           /* factor on the diffuse term of a shadowed point */
#define HR_SHADOW_EPS 1e-3f      /* m, shadow-ray origin offset along the normal */
#define HR_LIGHT_X (2.0f / 7.0f) /* (2, -3, 6) / 7: unit length */
#define HR_LIGHT_Y (-3.0f / 7.0f)
#define HR_LIGHT_Z (6.0f / 7.0f)
#define HR_SKY_R 0.53f
#define HR_SKY_G 0.73f
#define HR_SKY_B 0.92f
#define HR_GROUND_EVEN 0.75f
#define HR_GROUND_ODD 0.55f
#define HR_BODY_R 0.80f          /* default body colour (hr_set_appearance with a NULL colour array) */
#define HR_BODY_G 0.68f
#define HR_BODY_B 0.52f

#define HR_SEG_MARKER 1000       /* segmentation id of a marker pixel */
#define HR_MAX_MARKERS 24        /* marker spheres per env */

/* hr_render flags */
#define HR_FLAG_SHADOWS 1u       /* bit 0: shadow rays */
#define HR_FLAG_CHECKER 2u       /* bit 1: two-grey ground checker */
#define HR_FLAG_NO_CULL 4u       /* bit 2: diagnostics -- every ray tests every primitive (the image is
                                    the same; tools/render_bench.py measures what culling buys) */
#define HR_FLAGS_DEFAULT (HR_FLAG_SHADOWS | HR_FLAG_CHECKER)

#define HR_FOLLOW_POSITION 0
#define HR_FOLLOW_TRANSFORM 1
#define HR_FOLLOW_POSITION_XY 2

/* One camera sensor (gymapi.CameraProperties + set_camera_location / attach_camera_to_body). */
typedef struct hr_camera {
    int32_t env;            /* the env whose bodies and markers it sees, in [0, num_envs) */
    int32_t width, height;  /* pixels; all cameras of one renderer share one size */
    float hfov_deg;         /* horizontal field of view, degrees, in (0, 180) */
    float near, far;        /* kept hits have near <= t <= far; near > 0 */
    int32_t follow_body;    /* -1: fixed; else the body of `env` the camera follows */
    int32_t follow_mode;    /* HR_FOLLOW_POSITION / HR_FOLLOW_TRANSFORM / HR_FOLLOW_POSITION_XY */
    float pos[3];           /* fixed: world point; following: offset from the body origin */
    float target[3];        /* likewise */
} hr_camera;

typedef struct hr_renderer hr_renderer;

const char* hr_last_error(void);
int hr_version(void);

/* Binds HIP device `device` and copies the model's geometry (geom_type, geom_params) to it. */
int hr_create(int device, const he_model* model, int num_envs, hr_renderer** out);
int hr_destroy(hr_renderer* h);

/* The host-side check hr_set_cameras applies (no device needed): non-zero, with the reason in
 * hr_last_error(), for k < 1, a null array, a non-positive width, height, fov (or one >= 180) or near
 * plane, far < near, cameras of differing size, an env outside [0, num_envs), a follow_body outside
 * [-1, 24) or a follow_mode outside 0..2. */
int hr_validate_cameras(const hr_camera* host_cams, int k, int num_envs);

/* Replaces the renderer's camera set by host_cams[0..k) (HOST array, copied). A refused set leaves
 * the previous one in place and launches nothing. */
int hr_set_cameras(hr_renderer* h, const hr_camera* host_cams, int k);

/* set_rigid_body_color / set_rigid_body_segmentation_id: body_rgb f32 [N,24,3] in [0,1], body_seg i32
 * [N,24], DEVICE arrays read at render time. NULL: HR_BODY_* for every body / segmentation id 0. */
int hr_set_appearance(hr_renderer* h, const float* body_rgb, const int32_t* body_seg);

/* Marker spheres (the reference draws its motion targets as marker actors, render_env.py:306-335):
 * pos f32 [N,m,3] world points, DEVICE array read at render time; host_rgb f32 [m,3] HOST array,
 * copied; one radius > 0 for all. 0 <= m <= HR_MAX_MARKERS; m = 0 removes them (pos, host_rgb unused). */
int hr_set_markers(hr_renderer* h, const float* pos, int m, const float* host_rgb, float radius);

/* Draws every camera in one launch. rb_state: the engine's f32 [N*24,13] buffer. Outputs for K cameras
 * of H x W pixels: color u8 [K,H,W,4], depth f32 [K,H,W], seg i32 [K,H,W]; a NULL output is not
 * written, at least one must be given. Non-zero without a camera set. */
int hr_render(hr_renderer* h, const float* rb_state, uint8_t* color, float* depth, int32_t* seg,
              uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HUMANOID_RENDER_H */
