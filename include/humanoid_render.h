/*
 * humanoid_render.h -- C ABI of libhumanoid_render.so, the headless camera sensors of the MI355X
 * (gfx950) humanoid engine: one HIP ray-casting kernel that draws the engine's analytic scene (24
 * sphere / capsule / box geoms per env on the env's terrain: the plane, a slope or box steps) straight
 * from the rigid-body state buffer that is already on the device, and a ray-cast sensor (height scans,
 * range fans) on the same scene. It replaces the camera-sensor half of Isaac Gym's graphics API as
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
 * xy jitter; drawing all of them would pile them up), that env's markers, and that env's terrain
 * (hr_set_terrain: the engine's per-env terrain option; kind 1 is the slope, kind 2 the steps, any other
 * value, or no kind array, the plane z = 0). Body b (row p, q of rb_state) carries one geom, given in
 * the body frame by the model:
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
 *   ground (plane):  when d_z < 0 and o_z > 0:  t = -o_z / d_z, normal (0,0,1).
 *   ground (slope):  sn = sinf(slope), cs = cosf(slope), taken once on the host in float32;
 *                    n = (-sn, 0, cs);  when d.n < 0 and o.n > 0:  t = -(o.n) / (d.n), normal n.
 *   ground (steps):  L = step_length, S = step_height. Cell c(x) = max(floor(x / L), 0): cell 0 is all
 *                    of x < L. Height h_c = S c; the solid is z <= h_c(x). A ray with o_z <= h_c(o_x)
 *                    has no ground hit. Otherwise the cells are walked from c = c(o_x), t0 = 0:
 *                    1. tread, when d_z < 0:  t = (h_c - o_z) / d_z,  x_t = o_x + t d_x;  a hit with
 *                       normal (0,0,1) when t >= t0 and x_t lies in the cell (x_t < L for cell 0, else
 *                       c L <= x_t < (c+1) L);
 *                    2. moving up, d_x > 0:  t_b = ((c+1) L - o_x) / d_x;  no ground hit when
 *                       t_b > far;  z_b = o_z + t_b d_z;  when z_b < h_(c+1) a riser hit at t_b with
 *                       normal (-1,0,0);  otherwise c += 1, t0 = t_b, again from 1;
 *                    3. moving down, d_x < 0:  no hit in cell 0;  otherwise t_b = (c L - o_x) / d_x,
 *                       no hit when t_b > far, otherwise c -= 1, t0 = t_b, again from 1 (a riser faces
 *                       -x and is never entered from above);
 *                    4. d_x = 0: no hit;
 *                    5. after HR_MAX_STEP_CELLS cells there is no ground hit.
 * A hit is kept when near <= t <= far. The nearest kept hit wins; candidates are visited in the order
 * ground, bodies 0..23, markers 0..m-1, and a later one replaces the current one only when its t is
 * strictly smaller.
 *
 * Outputs per pixel
 *   depth  -t (d.f): negative view-space distance, as Isaac Gym documents its depth image; -inf where
 *          nothing is hit. (Neither PhysX nor the Isaac renderer is available to pin this against.)
 *   seg    the body's segmentation id, HR_SEG_MARKER for a marker, 0 for ground (any terrain) and sky.
 *   colour sky: HR_SKY_*. Otherwise albedo (HR_AMBIENT + (1 - HR_AMBIENT) max(0, n.l) s) per channel,
 *          with the unit light direction l = (HR_LIGHT_X, HR_LIGHT_Y, HR_LIGHT_Z) (towards the
 *          light). s = HR_SHADOW when shadows are on, n.l > 0 and the shadow ray
 *          (o' = hit point + HR_SHADOW_EPS n, direction l) has an entry hit with t >= 0 on ANY of
 *          the 24 body geoms of the env (markers and the terrain cast no shadow; a ground point's
 *          shadow ray leaves along the terrain's normal n); otherwise s = 1.
 *          albedo: the body's colour; the marker's colour; the ground: with the checker on,
 *          HR_GROUND_EVEN when floor(x) + floor(y) of the hit point (o + t d) is even, HR_GROUND_ODD
 *          when odd (a grey, the same in all three channels); with it off, HR_GROUND_EVEN. A riser
 *          hit takes x = (c + 1/2) L, the middle of the tread below it (c the cell the ray left),
 *          in place of the hit point's x: its own x = (c+1) L is an integer for every fifth step
 *          of 0.4 m, where rounding would speckle the riser.
 *          Each channel c is clamped to [0, 1] and stored as (int)(c 255 + 0.5); alpha is 255.
 *          A pixel is 4 bytes R, G, B, A.
 *
 * THE RAY-CAST SENSOR (hr_set_rays, hr_cast_rays). R rays, the same for every env, in a frame attached
 * to one body (row p, q of rb_state) of each env. A ray (origin a, direction v, |v| = 1) becomes
 *   frame 0 (position):   o = p + a,          d = v;
 *   frame 1 (heading):    o = p + H a,        d = H v, with the heading of q: hx = rot(q, (1,0,0)),
 *                         l = sqrt(hx_x^2 + hx_y^2), (c, s) = (1, 0) when l < 1e-6, otherwise
 *                         (hx_x, hx_y) / l, and H w = (c w_x - s w_y, s w_x + c w_y, w_z);
 *   frame 2 (transform):  o = p + rot(q, a),  d = rot(q, v).
 * d is used as it comes out, not normalised again. The hits are those of the image with near = 0 and
 * far = max_range: entry hits only, the env's ground first, then bodies 0..23 (left out under
 * HR_RAYS_SKIP_BODIES), a later candidate replacing the current one only when its t is strictly
 * smaller. Markers are never hit. dist is t (+inf without a hit), hit is -2 without a hit, -1 for the
 * ground, else the body index.
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
#define HR_MAX_STEP_CELLS 512    /* cells of the steps a ray is walked through; after them, no ground hit */

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

/* The ground of each env. terrain_kind: DEVICE i32 [N] read at render time (the array given to
 * he_set_env_properties), or NULL: the plane in every env, and hr_render draws exactly what it draws
 * without this call. slope in radians; step_height >= 0; step_length > 0; all finite. A refused call
 * leaves the previous setting. Host floats and one borrowed pointer: no device call, no copy. */
int hr_set_terrain(hr_renderer* h, const int32_t* terrain_kind, float slope, float step_height, float step_length);

/* Draws every camera in one launch. rb_state: the engine's f32 [N*24,13] buffer. Outputs for K cameras
 * of H x W pixels: color u8 [K,H,W,4], depth f32 [K,H,W], seg i32 [K,H,W]; a NULL output is not
 * written, at least one must be given. Non-zero without a camera set. */
int hr_render(hr_renderer* h, const float* rb_state, uint8_t* color, float* depth, int32_t* seg,
              uint32_t flags, void* stream);

/* The ray-cast sensor (defined above). */
#define HR_MAX_RAYS 1024
#define HR_RAY_FRAME_POSITION 0   /* ray origin = body origin + origin, world axes */
#define HR_RAY_FRAME_HEADING 1    /* origin and direction rotated about z by the body's heading */
#define HR_RAY_FRAME_TRANSFORM 2  /* rotated by the body's rotation */
#define HR_RAYS_SKIP_BODIES 1u    /* hr_cast_rays flag: terrain only (a height scan does not see its own legs) */
typedef struct hr_ray { float origin[3]; float dir[3]; } hr_ray;   /* dir: unit length */

/* host_rays: HOST array of R rays, copied (a blocking upload, a setup call); the same for every env, in
 * a frame attached to `body` of each env. Refused (previous set kept): null, R outside 1..HR_MAX_RAYS,
 * body outside 0..23, mode outside 0..2, a component that is not finite, |dir| further than 1e-3 from 1. */
int hr_set_rays(hr_renderer* h, const hr_ray* host_rays, int R, int body, int frame_mode);

/* One launch for all envs. dist_out f32 [N,R]: t, +inf when nothing is hit within max_range; hit_out i32
 * [N,R]: -2 nothing, -1 terrain, else the body index; either may be NULL, not both. Refused before any
 * launch for a null handle or state, no output, unknown flag bits, max_range not finite or <= 0, or no
 * rays set. Does not synchronise the host. */
int hr_cast_rays(hr_renderer* h, const float* rb_state, float max_range, float* dist_out, int32_t* hit_out,
                 uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HUMANOID_RENDER_H */
