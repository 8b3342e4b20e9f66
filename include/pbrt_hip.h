/*
 * pbrt_hip.h -- C-ABI of libpbrt_hip.so, the MI355X (gfx950) Monte-Carlo ray-transport engine.
 *
 * This is the drop-in boundary of the hot path.  The reference
 * (ReaganCardoza/Physics-Based-Ray-Tracing) has NO FFI: its boundary is the Mitsuba-3 Python
 * plugin API.  Each entry point below therefore cites the reference *Python* interface it
 * replaces (file:line relative to the reference root); the Python mirror of that interface
 * lives in physics-based-ray-tracing_amd/ and reaches this library through ctypes only.
 *
 * Conventions
 *  - extern "C", plain pointers + sizes, no C++/torch types.
 *  - every function returns int: 0 = OK, <0 = error class (PBRT_E_*); the message is available
 *    from pbrt_last_error().  Nothing throws or exits across the ABI.
 *  - batched leaf ops take HOST pointers to C-contiguous SoA arrays ([component][n], f32/u32);
 *    the library stages them through its own device buffers.
 *  - *_dev variants take DEVICE pointers (e.g. torch tensor data_ptr(), or pbrt_dev_alloc) and keep data in HBM.
 *  - one pbrt_ctx per device; calls on a ctx are not re-entrant; calls are synchronous on return (the ctx
 *    stream has been synchronised) EXCEPT the image-formation *_dev entry points of ABI 5
 *    (pbrt_das_beamform_dev, pbrt_envelope_dev, pbrt_log_compress_dev, pbrt_us_apply_pulse_dev), pbrt_us_acquire_queue_dev,
 *    pbrt_scene_update_material and pbrt_dev_upload: those queue their work on the ctx stream, in call order behind everything queued before,
 *    and return; pbrt_ctx_synchronize / pbrt_dev_download wait for it.  A caller that hands in memory of
 *    another runtime's stream (a torch tensor) orders the two streams itself.
 *  - the caller owns every buffer it passes; the library owns device memory behind the opaque
 *    handles and retains no caller pointer past a call.
 */
#ifndef PBRT_HIP_H
#define PBRT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBRT_ABI_VERSION 5

/* ---- error classes ------------------------------------------------------------------------ */
#define PBRT_OK 0
#define PBRT_E_INVALID (-1) /* bad argument / inconsistent descriptor            */
#define PBRT_E_DEVICE (-2)  /* HIP runtime error (no device, launch failure ...) */
#define PBRT_E_NOMEM (-3)   /* host or device allocation failed                  */
#define PBRT_E_UNSUPPORTED (-4)

/* ---- primitives --------------------------------------------------------------------------- */
/* One 64-byte record per primitive.  World space, f32.
 *   TRIANGLE       g = v0[3], e1 = v1-v0 [3], e2 = v2-v0 [3], n = normalize(e1 x e2) [3]
 *   SPHERE         g = centre[3], radius, 8 x 0
 *   PARALLELOGRAM  g = corner[3], e1[3], e2[3], n[3]   (Mitsuba 'rectangle' under to_world:
 *                  corner = T(-1,-1,0), e1 = T(1,-1,0)-corner, e2 = T(-1,1,0)-corner)
 *   CONE           g = row-major 3x4 world -> object matrix of the closed unit cone (apex (0,0,1), base disc of
 *                  radius 1 in z = 0): any affine to_world, e.g. the 0.06 / 0.06 / 0.10 scale of
 *                  MitsubaScenes/Cone_Box.xml:36-47.  Hits report u = 0 (lateral surface) / 1 (base disc), v = 0.
 *   CYLINDER       g = row-major 3x4 world -> object matrix of the OPEN unit tube x^2 + y^2 = 1, 0 <= z <= 1 (no caps;
 *                  Mitsuba 'cylinder': object -> world = to_world * translate(p0) * to_frame((p1-p0)/L) *
 *                  scale(radius, radius, L), L = |p1 - p0|).  Orientation is the sign of det(3x3 part): > 0 normals
 *                  point away from the axis, < 0 towards it (flip_normals; the tube is symmetric under x -> -x, so the
 *                  host mirrors object x to pick the sign).  Hits report u = v = 0.
 * The scenes that feed these: scenes/cbox.xml (12 triangles + 2 spheres), scenes/simple.xml
 * (teapot.ply, 2256 triangles), MitsubaScenes/ *.xml (sphere / rectangle / cone), RayTracingV0.py (cylinder),
 * TestRing/TestRing.obj (1152 triangles).
 */
#define PBRT_PRIM_TRIANGLE 0u
#define PBRT_PRIM_SPHERE 1u
#define PBRT_PRIM_PARALLELOGRAM 2u
#define PBRT_PRIM_CONE 3u /* analytic; cannot carry an area emitter (like SPHERE) */
#define PBRT_PRIM_CYLINDER 4u /* analytic; cannot carry an area emitter (like SPHERE) */

typedef struct pbrt_prim {
    float g[12];
    uint32_t type;     /* PBRT_PRIM_*                                   */
    uint32_t material; /* index into pbrt_scene_desc.materials          */
    int32_t emitter;   /* index into pbrt_scene_desc.emitters, -1: none */
    uint32_t shape;    /* caller's shape id (returned untouched)        */
} pbrt_prim;

/* ---- materials (BSDFs) -------------------------------------------------------------------- */
/* DIFFUSE     p[0..2] = reflectance                      (Mitsuba 'diffuse', scenes/cbox.xml:36-50)
 * CONDUCTOR   p[0..2] = specular_reflectance, perfect mirror (Mitsuba 'conductor' default,
 *                                                          scenes/cbox.xml:54)
 * DIELECTRIC  p[0] = eta = int_ior / ext_ior             (Mitsuba 'dielectric', scenes/cbox.xml:52)
 * ULTRA       p[0] = impedance, p[1] = roughness, p[2] = medium_z (1.2)
 *                                                        (UltraBSDF, CustomBSDF.py:7-26,105)
 * NONE        absorbs everything
 * ROUGHCONDUCTOR      p[0] = alpha, p[1..3] = eta (r, g, b), p[4..6] = k (r, g, b): isotropic GGX microfacet conductor with
 *                     visible-normal sampling (Mitsuba 'roughconductor', distribution 'ggx', sample_visible true).  eta = 0,
 *                     k = 1 is Mitsuba's material 'none': Fresnel reflectance exactly 1
 * CONDUCTOR_FRESNEL   p[1..3] = eta, p[4..6] = k: smooth conductor, a delta lobe of weight F(cos theta_i) per channel
 *                     (Mitsuba 'conductor' given eta / k)
 * Records of the last two types are checked by pbrt_scene_create / pbrt_scene_update_material / the BSDF leaf operators:
 * PBRT_E_INVALID unless alpha is finite and > 0 and every eta, k is finite and >= 0.  An alpha below 1e-3 is used as 1e-3.
 */
#define PBRT_MAT_DIFFUSE 0u
#define PBRT_MAT_CONDUCTOR 1u
#define PBRT_MAT_DIELECTRIC 2u
#define PBRT_MAT_ULTRA 3u
#define PBRT_MAT_NONE 4u
#define PBRT_MAT_ROUGHCONDUCTOR 5u
#define PBRT_MAT_CONDUCTOR_FRESNEL 6u

typedef struct pbrt_material {
    uint32_t type;
    float p[7];
} pbrt_material;

/* ---- emitters ----------------------------------------------------------------------------- */
/* AREA   radiance; its primitives are light_prims[first .. first+count) with the inclusive,
 *        normalised area CDF light_cdf[first .. first+count); area = summed surface area.
 * POINT  radiance = intensity, pos = position.
 */
#define PBRT_EMIT_AREA 0u
#define PBRT_EMIT_POINT 1u

typedef struct pbrt_emitter {
    uint32_t type;
    float radiance[3];
    float pos[3];
    uint32_t first;
    uint32_t count;
    float area;
    float pad[2];
} pbrt_emitter;

#define PBRT_ACCEL_AUTO 0u  /* brute force when n_prims <= 32, LDS-resident BVH otherwise */
#define PBRT_ACCEL_BRUTE 1u /* uniform loop over all primitives (scalar loads)            */
#define PBRT_ACCEL_BVH 2u   /* BVH4 (child boxes on an 8-bit grid, 40-byte leaf records), nodes + leaf records staged into LDS per
                               workgroup (read through the vector caches when the image does not fit the 160 KB of LDS)   */
#define PBRT_ACCEL_BVH_GLOBAL 3u /* BVH4 read through the vector caches even if it would fit LDS (the kernel variant of
                               large meshes, forced: for tests and A/B runs)                 */

typedef struct pbrt_scene_desc {
    uint32_t n_prims;
    const pbrt_prim *prims;
    uint32_t n_materials;
    const pbrt_material *materials;
    uint32_t n_emitters;
    const pbrt_emitter *emitters;
    uint32_t n_light_prims;
    const uint32_t *light_prims;
    const float *light_cdf;
    uint32_t accel; /* PBRT_ACCEL_* */
    /* optional, [n_prims][9]: the vertex normals n0, n1, n2 (world space, unit length) of a primitive of a mesh that has
     * them: the shading normal of a hit is si.sh_frame.n = normalize(b0 n0 + b1 n1 + b2 n2) (Mitsuba Mesh), the geometric
     * normal g[9..11] stays the one rays are offset along.  A PARALLELOGRAM row holds one normal three times (a merged
     * quad keeps its vertex normals only if they all agree).  All-zero row, or NULL: the face normal. */
    const float *vertex_normals;
} pbrt_scene_desc;

/* ---- camera / film (radiance mode) -------------------------------------------------------- */
/* Mitsuba 'perspective' sensor (scenes/cbox.xml:11-21, scenes/simple.xml:7-12).
 * to_world: row-major 3x4 camera-to-world matrix; columns are (left, up, dir, origin).  */
typedef struct pbrt_camera {
    float to_world[12];
    float tan_half_fov_x;
    float near_clip;
    float far_clip;
    uint32_t film_w; /* full film size; crops are given per render call */
    uint32_t film_h;
} pbrt_camera;

#define PBRT_FILTER_BOX 0u      /* radius 0.5 (scenes/simple.xml:17) */
#define PBRT_FILTER_TENT 1u     /* radius 1.0 (scenes/cbox.xml:28)   */
#define PBRT_FILTER_GAUSSIAN 2u /* stddev 0.5, radius 2.0            */

typedef struct pbrt_film_desc {
    uint32_t crop_x, crop_y, crop_w, crop_h; /* output window inside the full film      */
    uint32_t spp;                            /* samples per pixel rendered by this call  */
    uint32_t sample_offset;                  /* index of the first sample (RNG key)      */
    uint32_t max_depth;                      /* Mitsuba path 'max_depth' (cbox.xml:4,8)  */
    uint32_t rr_depth;                       /* Mitsuba path 'rr_depth' (default 5)      */
    uint32_t filter;                         /* PBRT_FILTER_*                            */
    uint32_t seed;
    uint32_t flags;      /* PBRT_FILM_*                                                  */
    uint32_t pass_paths; /* 0 = library default; paths kept in flight per pass.  Default: 64 Mi for brute-force scenes
                            (8 B..120 B of workspace per path, by launch plan); BVH scenes (340 B per path) the largest power of
                            two, 1 .. 512 Mi, whose workspace fits two thirds of the free device memory -- pbrt_stats reports both */
} pbrt_film_desc;

#define PBRT_FILM_RAW_ACCUM 1u /* output 4 floats/pixel (sum w*rgb, sum w) un-normalised: \
                                  for sample-sharded multi-GPU reduction */
/* The flags marked DIAGNOSTIC BUILD select launch structures that lost their A/B: the product library does not carry their kernels
 * and refuses them with PBRT_E_UNSUPPORTED; libpbrt_hip_diag.so (make -C csrc diag, -DPBRT_DIAG) has them (kernels: csrc/kernels_diag.h,
 * host side: csrc/diag_driver.h).  Same film either way. */
#define PBRT_FILM_NO_REPACK 2u /* DIAGNOSTIC BUILD, with PBRT_FILM_NO_HIT_POOL: do not re-densify the live paths before bounces >= 2 */
#define PBRT_FILM_FUSE_PLAN_SET 0x80u /* bits 8..15 of flags hold the fuse plan: bit d set = the launch that walks bounce d goes on \
                                        with bounce d + 1 of its paths in registers, up to 6 bounces per launch (brute-force \
                                        kernels; same film whatever the plan).  PBRT_FILM_FUSE_PLAN(0) = one launch per bounce, \
                                        (0x15) = pairs, (0xff) = six bounces per launch.  Unset: the library chooses from how many \
                                        paths survive each bounce (it goes on while >= 45 % do) -- measured on a 2-spp probe \
                                        pass at the start of the first render of a scene, afterwards on the scene's last render */
#define PBRT_FILM_FUSE_PLAN(mask) (PBRT_FILM_FUSE_PLAN_SET | (((mask) & 0xffu) << 8))
#define PBRT_FILM_WALK_SET 0x10000u /* DIAGNOSTIC BUILD: bits 17..24 of flags hold the depth from which ONE launch walks every remaining \
                                       bounce of a pass (k_walk, brute-force kernels: the workgroup that owns a segment carries its \
                                       survivors on; 0 = one launch per pass, 0xff = never) */
#define PBRT_FILM_WALK_FROM(d) (PBRT_FILM_WALK_SET | (((d) & 0xffu) << 17))
#define PBRT_FILM_REGEN 8u /* DIAGNOSTIC BUILD: brute-force scenes, persistent waves with path regeneration (k_regen: no path state in \
                             memory, one launch per pass; measured slower than the wavefront launches) */
#define PBRT_FILM_NO_HIT_POOL 0x10u /* DIAGNOSTIC BUILD: BVH scenes through the fused bounce kernel (closest hit, shading and shadow ray in \
                                    one launch per bounce, 4 waves per SIMD) instead of k_trace + k_shade (kernels_wavefront.h) */
#define PBRT_FILM_NO_OCCLUDER_PRUNING 4u /* diagnostic: next-event shadow segments of brute-force scenes walk EVERY primitive \
                                           instead of the occluder list (DESIGN D11: primitives on the scene's convex hull \
                                           and the lone area light are left out of it) -- same film if the pruning is right */
#define PBRT_FILM_NO_TILE_CULL 0x20u /* diagnostic: the camera rays of brute-force scenes walk EVERY primitive instead of the ones the \
                                        keep word of their 8 x 8 pixel tile leaves (csrc/tile_cull.h) -- same film if the culling is right */
#define PBRT_FILM_NO_ORDERED_WALK 0x40u /* diagnostic: a brute-force scene whose primitive lists are class-ordered (parallelograms, then \
                                           triangles, then curved records) is rendered through the kernels that walk the run tables \
                                           (csrc/prim_runs.h) -- same film, same statistics */
#define PBRT_FILM_NO_PATH_KERNEL 0x2000000u /* diagnostic: a pass of camera paths whose every bounce one launch walks (brute-force \
                                               scenes without glossy materials, max_depth <= 6) goes through the bounce kernel with \
                                               its survivor compaction instead of k_path (csrc/kernels_radiance.h) -- same film, \
                                               same statistics */

/* ---- ultrasound (acoustic) mode ----------------------------------------------------------- */
/* Parameter block of UltraIntegrator (CustomIntegrator.py:13-48) plus the sensor transform
 * the integrator reads from scene.sensors()[0].transform (CustomIntegrator.py:272). */
#define PBRT_US_MAX_ANGLES 64

/* CustomEmitter (CustomEmmitter.py:5-49), linear or convex array. */
typedef struct pbrt_us_emitter {
    uint32_t number_of_elements;
    float pitch, element_width, element_height;
    float radius;        /* 0: linear */
    float opening_angle; /* degrees   */
    uint32_t number_of_rays_per_element;
    float speed_of_sound;
    float steering_angle_min, steering_angle_max; /* degrees */
} pbrt_us_emitter;

/* Where the primary ray of a path comes from (pbrt_us_params.primary).
 * ELEMENT  the integrator's own deterministic ray, CustomIntegrator.py:264-273: origin T (x_e, 0, 0), direction
 *          normalize(T (sin theta_a, 0, cos theta_a)), emission time tx_delay[a, e], amplitude 1.  All paths of an (angle, element)
 *          pair share it (which is what the first-bounce tables exploit).
 * EMITTER  every path draws its own ray from CustomEmitter.sample_ray (CustomEmmitter.py:81-107, pbrt_us_params.emitter) -- what
 *          BASELINE config 3 "with CustomBSDF + CustomEmmitter" means read literally.  The reference never connects the two classes
 *          (its integrator does not call the emitter), so the connection is a definition of this library: the
 *          (angle, element) grid of the acquisition stratifies the emitter's sample space -- path k of pair (a, e) calls
 *              sample_ray(time = 0, sample1 = (e + 1/2) / N, sample2 = (u.x, u.y), sample3 = (a + u.z) / n_angles)
 *          with u = the path's RNG block 0x80000000, i.e. element e (jittered inside the element by sample2, :64-68) and a steering
 *          angle drawn uniformly from the a-th of n_angles equal parts of [steering_angle_min, steering_angle_max] (:85-87); the
 *          ray is taken to the world with the sensor transform like the integrator's own (:272-273), its `time` (the element's
 *          steering delay -x sin(psi) / c, :93-94) is the path's initial time of flight (t0 of :329 is then 0) and its weight
 *          max(0, d.n) / N_total_rays (:97-98) multiplies every echo the path deposits -- as Mitsuba's render loop multiplies what
 *          Integrator.sample returns by the weight of the sampled ray; the path's own amplitude starts at 1 (:276), so the
 *          Russian roulette of :364-367, which reads that amplitude as a survival probability, is the integrator's.
 *          emitter.number_of_elements must equal n_elements.  No first-bounce tables: every path walks the scene from its own
 *          origin. */
#define PBRT_US_PRIMARY_ELEMENT 0u
#define PBRT_US_PRIMARY_EMITTER 1u
/* The convex (curved) array, OR-ed into pbrt_us_params.primary beside PBRT_US_PRIMARY_ELEMENT or _EMITTER.  The
 * reference's integrator knows no curved array; these statements are this library's definition.
 * Geometry   CustomEmitter's, literally (CustomEmmitter.py:41-47), in the sensor's local frame and read from pbrt_us_params.emitter:
 *            the centre of curvature is the origin, theta_e = linspace(-span / 2, +span / 2, N) with span = opening_angle in radians
 *            (`pitch` is not read), element e sits at (R sin theta_e, 0, R cos theta_e) with normal (sin theta_e, 0, cos theta_e);
 *            the apex is (0, 0, R).  emitter.radius must be finite and > 0, emitter.opening_angle finite, > 0 and < 180,
 *            emitter.number_of_elements == n_elements: PBRT_E_INVALID otherwise.  pbrt_us_array_elements returns the table
 *            (x, z, nx, nz) per element that the kernels read; sin / cos of theta_e are the emitter's own (so the position a ray is
 *            emitted from and the position the receive connection aims at are the same floats up to |theta_e| = 45 degrees; beyond,
 *            host and device library sin / cos may differ in the last bits).
 * Delays     tx[a, e] = (x_e sin theta_a + (z_e - R) cos theta_a) / c: the plane wave along (sin theta_a, 0, cos theta_a), referenced
 *            to the apex.  For R -> inf with the apex held fixed this is the linear x_e sin theta_a / c.  pbrt_us_tx_delays honours the
 *            bit, and the tx_delays an acquisition returns are this table.
 * ELEMENT    the primary ray starts on the arc: origin T (x_e, 0, z_e), direction normalize(T (sin theta_a, 0, cos theta_a)),
 *            amplitude 1, emission time tx[a, e].
 * EMITTER    unchanged: CustomEmitter.sample_ray is convex by itself when radius != 0.
 * Receive    the connection (CustomIntegrator.py:320-322) aims at T (x_r, 0, z_r), and the directivity angle (:289-304) is taken against
 *            the receive element's own normal, normalize(T (nx_r, 0, nz_r)).  Everything else keeps the array axis T (0, 0, 1): the
 *            cut-off cone of :371, w_o, the roulette, quirks and RNG blocks.
 * Without the bit, PBRT_US_PRIMARY_EMITTER with emitter.radius != 0 (transmit from an arc, receive on a line: never defined) is
 * refused with PBRT_E_UNSUPPORTED.  No struct changes size; a library from before D18 refuses the bit (PBRT_E_INVALID).
 * Kernels: instances of their own; they read the behaviour switches at run time (no compiled-in quirk set). */
#define PBRT_US_ARRAY_CONVEX 0x100u

typedef struct pbrt_us_params {
    uint32_t max_depth;    /* CustomIntegrator.py:16 */
    float frequency;       /* :17 */
    float sound_speed;     /* :18 */
    float attenuation;     /* :19 */
    float main_beam_angle; /* degrees, :21 */
    float cutoff_angle;    /* degrees, :22 */
    float fs;              /* 'sampling_rate', :23 */
    uint32_t n_elements;   /* :26 */
    float pitch;           /* :27 */
    uint32_t n_angles;     /* :33-34 */
    float angles_deg[PBRT_US_MAX_ANGLES];
    uint32_t time_samples; /* :42 */
    float sensor_to_world[12]; /* row-major 3x4 */
    float max_path_len;        /* hard-coded 0.2 in the reference (:307,372) */
    uint32_t quirks;           /* PBRT_USQ_* */
    uint32_t primary;          /* PBRT_US_PRIMARY_* (ABI 5), | PBRT_US_ARRAY_CONVEX */
    pbrt_us_emitter emitter;   /* read with PBRT_US_PRIMARY_EMITTER; with PBRT_US_ARRAY_CONVEX its radius, opening_angle, number_of_elements */
} pbrt_us_params;

/* Behaviour switches; each bit reproduces one reference quirk.
 * The library default (quirks = PBRT_USQ_REFERENCE) is the literal arithmetic of the scalar
 * variant simulate_acquisition_parallel (CustomIntegrator.py:235-376) and UltraBSDF.sample
 * (CustomBSDF.py:87-175) with ONE repair: 'survive' is initialised to True (quirk B5), because
 * as checked in the loop raises UnboundLocalError on the first surviving bounce. */
#define PBRT_USQ_DIAG_SAMPLE 0x1u   /* A2: scalar sample broadcast to Point2f(s,s)             */
#define PBRT_USQ_REF_REFLECT 0x2u   /* A5: reflected = wi + 2 cos m (not the mirror direction) */
#define PBRT_USQ_UNIT_GGX_PDF 0x4u  /* A7: ggx_pdf == 1.0                                       */
#define PBRT_USQ_DOUBLE_LOCAL 0x8u  /* A1: Frame(n).to_local applied to the already-local wi   */
#define PBRT_USQ_MIXED_FRAMES 0x10u /* A8: world shading normal dotted with local wi           */
#define PBRT_USQ_NEVER_ENTER 0x20u  /* A4: 'entering' is always false                          */
#define PBRT_USQ_CLAMP_TIME 0x40u   /* B3 (Dr.Jit variant): clamp t_idx instead of dropping    */
#define PBRT_USQ_NO_TOF_ACCUM 0x80u /* B2 (Dr.Jit variant): tof never accumulates              */
#define PBRT_USQ_NO_CARRIER 0x100u  /* f-3 pulse model: deposit atten*amp*w_i*w_o without the sin(phase) factor of :348; the carrier
                                       comes from pbrt_us_apply_pulse (not a reference quirk)  */
#define PBRT_USQ_NO_FIRST_TABLES 0x200u /* diagnostic: every path walks the scene at its first bounce (same result) */
#define PBRT_USQ_NO_FUSED_BOUNCES 0x400u /* diagnostic: one launch per bounce instead of one per pass */
#define PBRT_USQ_FROZEN_DRAWS 0x800u  /* B1 (Dr.Jit variant): np.random.uniform is evaluated while dr.while_loop TRACES its body
                                         (CustomIntegrator.py:153,173-174,219), so every bounce of a ray reuses the draws of its
                                         first one: the RNG block of bounce b is block 0                              */
#define PBRT_USQ_SIGNED_RR 0x1000u    /* B5 (Dr.Jit variant, :219-224): rr_prob = min(atten * amp, 1) without the abs, survive
                                         iff u < rr_prob (strict), atten = survive ? atten / rr_prob : 0             */
/* the Dr.Jit variant simulate_acquisition (CustomIntegrator.py:60-232), on top of PBRT_USQ_REFERENCE */
#define PBRT_USQ_DRJIT_VARIANT (PBRT_USQ_CLAMP_TIME | PBRT_USQ_NO_TOF_ACCUM | PBRT_USQ_FROZEN_DRAWS | PBRT_USQ_SIGNED_RR)
#define PBRT_USQ_REFERENCE                                                                \
    (PBRT_USQ_DIAG_SAMPLE | PBRT_USQ_REF_REFLECT | PBRT_USQ_UNIT_GGX_PDF | PBRT_USQ_DOUBLE_LOCAL | \
     PBRT_USQ_MIXED_FRAMES | PBRT_USQ_NEVER_ENTER)

/* UltraSensor (bytecode-only class; props used at USMain.py:43-65 and
 * MitsubaScenes/Sphere_Box.xml:16-34). */
typedef struct pbrt_us_sensor {
    uint32_t num_elements;
    float element_width, element_height, pitch;
    float radius; /* +inf: linear array */
    float center_frequency, sound_speed, directivity;
    float to_world[12];
} pbrt_us_sensor;

/* CustomSensor.put_data accumulator (CustomSensor.py:7-59). */
typedef struct pbrt_us_receiver {
    uint32_t number_of_elements;
    float pitch;
    float sample_rate;
    uint32_t time_samples;
} pbrt_us_receiver;

typedef struct pbrt_stats {
    uint64_t samples;      /* camera / transducer paths started by the last call           */
    uint64_t segments;     /* path segments shaded (sum over bounces of live paths)         */
    uint64_t shadow_rays;  /* occlusion rays                                               */
    double kernel_ms;      /* device time of the last call, HIP events on the ctx stream    */
    double bounce_ms;      /* of which: the dominant (bounce) kernels                       */
    uint32_t bounce_launches;
    uint32_t passes;
    uint64_t model_bytes;  /* algorithmic HBM bytes of the last call (DESIGN.md byte model) */
    uint64_t bounce_model_bytes;
    uint64_t live[16];     /* paths entering depth d (d = 0..15), summed over passes          */
    /* how the last call was launched (ABI 3).  The launch plan of a brute-force scene is state of the pbrt_scene: unless the
     * caller sets one (PBRT_FILM_FUSE_PLAN) it is learnt from the path survival of the scene's previous render, so TIMINGS depend
     * on the call history of a scene -- films never do. */
    uint32_t fuse_plan;    /* bit d: the launch that walks bounce d goes on with bounce d + 1 (brute-force scenes; 0 for BVH scenes) */
    uint32_t plan_source;  /* PBRT_PLAN_* */
    uint64_t pass_paths;   /* paths in flight per pass */
    uint64_t workspace_bytes; /* device memory the context holds after the call */
    uint64_t trace_model_bytes; /* ABI 4, BVH scenes: the part of bounce_model_bytes that belongs to the k_trace launches (the rest is k_shade's) */
} pbrt_stats;
#define PBRT_PLAN_CALLER 0u  /* pbrt_film_desc.flags carried PBRT_FILM_FUSE_PLAN */
#define PBRT_PLAN_LEARNT 1u  /* from the path survival of the scene's previous render */
#define PBRT_PLAN_PROBED 2u  /* first render of the scene: from a 2-spp probe pass at the start of this call */
#define PBRT_PLAN_DEFAULT 3u /* first render, too few samples for a probe: the library default (pairs) */
#define PBRT_PLAN_STREAMS 4u /* BVH scenes: one k_trace + one k_shade launch per bounce */

typedef struct pbrt_ctx pbrt_ctx;
typedef struct pbrt_scene pbrt_scene;

/* ---- context / scene ---------------------------------------------------------------------- */
int pbrt_abi_version(void);
/* replaces: mi.set_variant(...) (USMain.py:12) -- selects the device instead of a JIT backend */
int pbrt_ctx_create(int device, pbrt_ctx **out);
int pbrt_ctx_destroy(pbrt_ctx *ctx);
const char *pbrt_last_error(pbrt_ctx *ctx); /* ctx may be NULL: last ctx-less error */
int pbrt_get_stats(pbrt_ctx *ctx, pbrt_stats *out);
/* Workspace policy (ABI 4).  A context keeps the device buffers of its calls (path state, ray and radiance records, film
 * accumulators) and re-uses them; pbrt_stats.workspace_bytes says how much it holds.  BVH scenes size a pass to the largest power
 * of two of paths (1 .. 512 Mi, 340 B each) that fits two thirds of the free device memory -- up to 183 GB on an idle MI355X
 * (larger passes are faster: their twelve launches per pass fill the chip longer).  A caller
 * that shares the device (the reference's driver imports torch beside the renderer, USMain.py:5) bounds that with a limit -- here,
 * or PBRT_WORKSPACE_LIMIT_BYTES in the environment at pbrt_ctx_create; 0 = none -- and hands memory back with pbrt_ctx_trim.
 * Under a limit, and when an allocation fails, renders take smaller passes (same film, more passes); a request that cannot be met
 * at the smallest pass returns PBRT_E_NOMEM.  pbrt_film_desc.pass_paths still overrides the choice per call. */
int pbrt_ctx_set_workspace_limit(pbrt_ctx *ctx, uint64_t bytes); /* a limit below what the context holds frees its buffers at once */
/* frees every workspace buffer the most recent call did not use and every one larger than that call needed; *held_after
 * (may be NULL) = bytes still held */
int pbrt_ctx_trim(pbrt_ctx *ctx, uint64_t *held_after);

/* replaces: mi.load_dict / mi.load_file scene instantiation + accel build (USMain.py:257) */
int pbrt_scene_create(pbrt_ctx *ctx, const pbrt_scene_desc *desc, pbrt_scene **out);
/* replaces: params[key] = v; params.update() (USMain.py:264-265) -> BSDF.parameters_changed
 * (CustomBSDF.py:186-191).  Overwrites material `index` in place, no accel rebuild. */
int pbrt_scene_update_material(pbrt_scene *scene, uint32_t index, const pbrt_material *m);
int pbrt_scene_destroy(pbrt_scene *scene);

/* ---- the hot path: radiance mode ----------------------------------------------------------- */
/* replaces: mi.render(scene) == SamplingIntegrator::render -> Sensor.sample_ray ->
 * Integrator.sample (CustomIntegrator.py:52-53 is the stub; semantics SURVEY.md App. D) ->
 * film.  out_rgb: host float[crop_h*crop_w*3] (or *4 with PBRT_FILM_RAW_ACCUM). */
int pbrt_render_radiance(pbrt_scene *scene, const pbrt_camera *cam, const pbrt_film_desc *film, float *out_rgb);
/* same, output left in HBM at device pointer d_out (no PCIe copy) */
int pbrt_render_radiance_dev(pbrt_scene *scene, const pbrt_camera *cam, const pbrt_film_desc *film, void *d_out);

/* replaces: Integrator.sample(scene, sampler, ray, medium, active) -> (spec, mask, aovs)
 * (CustomIntegrator.py:52-53 is a stub returning 0; radiance semantics SURVEY.md App. D).
 * Radiance arriving along n caller-supplied rays: o,d [3][n] (unit d), tmax [n]; the RNG key of ray i
 * is (index_offset + i, sample_index).  out rgb [3][n]. */
int pbrt_integrator_sample(pbrt_scene *scene, uint32_t n, const float *o, const float *d, const float *tmax,
                           uint32_t index_offset, uint32_t sample_index, uint32_t seed, uint32_t max_depth,
                           uint32_t rr_depth, float *rgb);

/* ---- the hot path: ultrasound mode ---------------------------------------------------------- */
/* replaces: UltraIntegrator.simulate_acquisition_parallel(scene) (CustomIntegrator.py:235-405),
 * called from USMain.py:99.  Traces paths k in [path_offset, path_offset+paths_per_ray) for
 * every (angle, element) pair; channel_buf[(a*n_elements+recv)*time_samples + t] accumulates the
 * echoes divided by norm_paths (pass the TOTAL paths per ray of the job so that shards sum to
 * the single-device result); tx_delays[a*n_elements+e] as CustomIntegrator.py:254-257. */
int pbrt_us_acquire(pbrt_scene *scene, const pbrt_us_params *p, uint32_t seed, uint32_t paths_per_ray,
                    uint32_t path_offset, uint32_t norm_paths, float *channel_buf, float *tx_delays);
int pbrt_us_acquire_dev(pbrt_scene *scene, const pbrt_us_params *p, uint32_t seed, uint32_t paths_per_ray,
                        uint32_t path_offset, uint32_t norm_paths, void *d_channel_buf, float *tx_delays);

/* ---- batched leaf operators (host SoA in/out) ---------------------------------------------- */
/* replaces: scene.ray_intersect(ray) (CustomIntegrator.py:146,309).  o,d: [3][n]; tmax: [n];
 * out t [n] (+inf: miss), prim [n] (0xffffffff: miss), u,v [n]. */
int pbrt_ray_intersect(pbrt_scene *scene, uint32_t n, const float *o, const float *d, const float *tmax, float *t,
                       uint32_t *prim, float *u, float *v);
/* replaces: scene.ray_intersect(si.spawn_ray(sec_dir)).is_valid() used as an occlusion test
 * (CustomIntegrator.py:159-160,324-325).  hit [n] is 0/1. */
int pbrt_ray_test(pbrt_scene *scene, uint32_t n, const float *o, const float *d, const float *tmax, uint8_t *hit);

/* replaces: BSDF.sample(ctx, si, sample1, sample2) (CustomBSDF.py:87-175 for ULTRA; Mitsuba
 * diffuse / conductor / dielectric per SURVEY.md App. D).
 *  wi      [3][n] incident direction in the local shading frame (si.wi)
 *  n_geo   [3][n] world geometric normal (si.n)        -- read by ULTRA only
 *  n_sh    [3][n] world shading normal (si.sh_frame.n) -- read by ULTRA only
 *  sh_s    [3][n] tangent of the shading frame (si.sh_frame.s, or the shape's dp_du: Mitsuba builds the frame as
 *                 s = normalize(dp_du - n (n . dp_du)), t = n x s) -- read by ULTRA only, for bs.wo = si.to_local(chosen)
 *                 (CustomBSDF.py:165); NULL: coordinate_system(n_sh)
 *  s1 [n], s2 [2][n] the uniform variates
 *  out: wo [3][n] local, pdf [n], weight [3][n] (ULTRA: amplitude in weight[0], rest equal),
 *       sampled [n]: 0 = reflection lobe, 1 = transmission lobe, 0xffffffff = invalid sample */
int pbrt_bsdf_sample(pbrt_ctx *ctx, const pbrt_material *m, uint32_t quirks, uint32_t n, const float *wi,
                     const float *n_geo, const float *n_sh, const float *sh_s, const float *s1, const float *s2, float *wo,
                     float *pdf, float *weight, uint32_t *sampled);
/* replaces: BSDF.eval / BSDF.pdf / BSDF.eval_pdf (CustomBSDF.py:177-184: constant 0 for ULTRA).
 * f [3][n] = bsdf value * cos(theta_o). */
int pbrt_bsdf_eval_pdf(pbrt_ctx *ctx, const pbrt_material *m, uint32_t n, const float *wi, const float *wo, float *f,
                       float *pdf);

/* Emitter.sample_direction(it, sample) -- required by the north star, absent from the
 * reference; semantics of Mitsuba area / point emitters.  No visibility test.
 *  p [3][n] reference points; u [4][n] variates (emitter pick, primitive pick, 2-D position)
 *  out: d [3][n], dist [n], pdf [n] (solid angle; 1 for delta), weight [3][n] = radiance/pdf,
 *       q [3][n] sampled point, emitter [n] */
int pbrt_emitter_sample_direction(pbrt_scene *scene, uint32_t n, const float *p, const float *u, float *d, float *dist,
                                  float *pdf, float *weight, float *q, uint32_t *emitter);

/* replaces: Sensor.sample_ray of the Mitsuba 'perspective' sensor. pos [2][n] in [0,1)^2 over
 * the full film.  out: o,d [3][n], tmax [n]. */
int pbrt_sensor_sample_ray(pbrt_ctx *ctx, const pbrt_camera *cam, uint32_t n, const float *pos, float *o, float *d,
                           float *tmax);

/* replaces: UltraSensor.sample_ray(time, wavelength_sample, position_sample, aperture_sample)
 * (SURVEY.md App. C).  time, wavelength_sample [n]; position_sample, aperture_sample [2][n].
 * use_hemisphere_warp != 0 selects the warp.square_to_uniform_hemisphere branch. */
int pbrt_us_sensor_sample_ray(pbrt_ctx *ctx, const pbrt_us_sensor *s, int use_hemisphere_warp, uint32_t n,
                              const float *time, const float *wavelength_sample, const float *position_sample,
                              const float *aperture_sample, float *o, float *d, float *weight);

/* replaces: CustomEmitter.sample_ray(time, sample1, sample2, sample3) (CustomEmmitter.py:81-107)
 * incl. sample_position (:51-79).  time, s1, s3 [n]; s2 [2][n].
 * out: o,d [3][n], ray_time [n], weight [n], pdf_pos [n]. */
int pbrt_us_emitter_sample_ray(pbrt_ctx *ctx, const pbrt_us_emitter *e, uint32_t n, const float *time,
                               const float *s1, const float *s2, const float *s3, float *o, float *d, float *ray_time,
                               float *weight, float *pdf_pos);

/* replaces: CustomSensor.put_data(ray, amplitude) (CustomSensor.py:29-59), batched: ray origin
 * x [n], ray time [n], ray direction [3][n], amplitude [n] accumulated into
 * channel_buffer[number_of_elements*time_samples] (host, read-modify-write). */
int pbrt_us_put_data(pbrt_ctx *ctx, const pbrt_us_receiver *r, uint32_t n, const float *ox, const float *time,
                     const float *d, const float *amplitude, float *channel_buffer);

/* tx_delay[a,e] = elem_x[e] * sin(theta_a) / c  (CustomIntegrator.py:246-257); host-only helper
 * shared by pbrt_us_acquire. */
int pbrt_us_tx_delays(const pbrt_us_params *p, float *tx_delays);
/* The elements of the array in the sensor's frame, elem[n_elements][4] = (x_e, z_e, nx_e, nz_e): the curved array of
 * PBRT_US_ARRAY_CONVEX, else the line (x_e, 0, 0, 1).  Host-only helper shared by pbrt_us_acquire; the table the *_probe forms of
 * the beamformer take.  PBRT_E_INVALID for a curved array whose parameters the acquisition would refuse. */
int pbrt_us_array_elements(const pbrt_us_params *p, float *elem);

/* ---- image formation behind the hot path ------------------------------------------
 * The reference hands the channel buffer to the third-party `ultraspy` package (absent here; parity unpinned):
 * DelayAndSum.beamform(data, GridScan(x, z)) -> compute_envelope -> manual log compression
 * (USMain.py:126-221).  These entry points are this build's own definition of those three steps. */
#define PBRT_DAS_NEAREST 0u
#define PBRT_DAS_LINEAR 1u
typedef struct pbrt_das_params {
    uint32_t n_angles, n_elements, time_samples; /* data [n_angles][n_elements][time_samples] (RF, f32) */
    float fs, sound_speed, t0;                   /* sample s was taken at t0 + s / fs */
    float f_number;                              /* receive element e used iff |x - x_e| <= z / (2 f_number); 0: all */
    uint32_t interpolation;                      /* PBRT_DAS_NEAREST / PBRT_DAS_LINEAR */
    uint32_t compound_mean;                      /* 0: sum over transmissions, 1: mean */
    uint32_t nx, nz;                             /* GridScan(x, z) */
} pbrt_das_params;

/* replaces: ultraspy DelayAndSum.beamform(d_data, scan) as called at USMain.py:204.
 * out[ix][iz] = sum_a sum_e data[a][e](t_tx(a; x, z) + |(x, z) - (elem_x[e], 0)| / c), where the transmit time is the
 * first arrival of the emitted wavefront, t_tx = min_e' (tx_delays[a][e'] + |(x, z) - (elem_x[e'], 0)| / c)  (equal to
 * (x sin(theta) + z cos(theta)) / c for the plane-wave delays of pbrt_us_tx_delays inside the aperture's shadow).
 * Sample positions are evaluated in f64 and kept as whole samples plus an f32 fraction; samples are interpolated and summed in f32
 * in the order (wave = e % 4, trip of 5 transmissions, element, transmission within the trip), the four waves' partial sums added
 * last.  Linear: floor(s) in [0, T - 1), or s == T - 1 exactly; nearest: round half to even into [0, T - 1].  The tests hold every
 * pixel to (n_terms + 16) 2^-24 sum_terms max(|v0|, |v1|) of an f64 evaluation (tests/das_util.py), and constant traces to the
 * exact sum.  Host pointers. */
int pbrt_das_beamform(pbrt_ctx *ctx, const pbrt_das_params *p, const float *data, const float *tx_delays,
                      const float *elem_x, const float *x, const float *z, float *out);
/* The same on an element table elem[n_elements][4] = (x_e, z_e, nx_e, nz_e) (pbrt_us_array_elements; a curved probe):
 * distances are |(x, z) - (x_e, z_e)| on the first-arrival and on the receive side, and the f-number aperture lies in the element's
 * frame -- with v = (x - x_e, z - z_e), depth d_n = v . n_e and lateral d_t = v x n_e, element e receives the pixel iff d_n > 0 and
 * 2 f_number |d_t| <= d_n (f_number <= 0: every element receives every pixel).  For n_e = (0, 1), z_e = 0 that is pbrt_das_beamform's
 * |x - x_e| <= z / (2 f_number).  Summation order, f64 sample positions and interpolation as above.  No tile of the scan is skipped
 * up front (the linear form leaves tiles outside the array's span early); an element outside every aperture of a tile still costs
 * no square root.  Same argument checks; the *_probe_dev forms below are queued and recordable like the forms they sit beside. */
int pbrt_das_beamform_probe(pbrt_ctx *ctx, const pbrt_das_params *p, const float *data, const float *tx_delays,
                            const float *elem, const float *x, const float *z, float *out);

/* replaces: ultraspy DelayAndSum.compute_envelope(d_output, scan) on RF data (USMain.py:205): modulus of the
 * analytic signal along the axial (z, fastest) axis, i.e. |scipy.signal.hilbert(rf, axis=-1)|.  nz <= 4096.
 * A column that holds a NaN or an infinity comes out NaN at every sample, as the FFT of the definition makes it; the other
 * columns are not affected.  Finite input gives the same bits whichever of the two kernels (odd / even nz) runs. */
int pbrt_envelope(pbrt_ctx *ctx, uint32_t nx, uint32_t nz, const float *rf, float *env);

/* replaces: the manual log compression of USMain.py:210-218: db = 20 log10(env + 1e-12), clipped to
 * [max(db) - dynamic_range_db, max(db)], mapped to [0, 1].  n values in, n values out.  As np.max does there, a NaN
 * propagates: if any value is NaN, or so negative that env + 1e-12f < 0, max(db) is NaN and every output is NaN. */
int pbrt_log_compress(pbrt_ctx *ctx, uint32_t n, const float *env, float dynamic_range_db, float *out);

/* SURVEY.md section 8 f-3, the pulse model of the reference's prototype (RayTracingV0.py:194-204, "UltraRay Eq. 14"):
 *   pulse(t; t0, amp) = amp * sin(2 pi fc (t - t0)) * exp(-(t - t0)^2 / sigma^2).
 * With echoes deposited as plain amplitudes on the sample grid (PBRT_USQ_NO_CARRIER) the RF trace is the discrete
 * convolution of every trace with h[k] = sin(2 pi fc k / fs) * exp(-(k / fs)^2 / sigma^2), |k| <= ceil(2.5 sigma fs):
 * out[tr][n] = sum_k in[tr][n - k] * h[k]  (zero outside the trace).  n_traces x time_samples values, host pointers;
 * in and out must not overlap (PBRT_E_INVALID).  [DEFINE] sigma = wave_cycles / (4 fc) turns the integrator's unused `wave_cycles`
 * (CustomIntegrator.py:20) into the pulse length. */
int pbrt_us_apply_pulse(pbrt_ctx *ctx, uint32_t n_traces, uint32_t time_samples, float fs, float frequency, float sigma,
                        const float *in, float *out);

/* ---- ABI 5: the reference's us_render loop without leaving HBM -------------------------------------------------------
 * USMain.py:92-252 runs acquisition -> DAS -> envelope -> log compression 51 times per script (:260, :279-283).  With the
 * host-pointer forms above every step crosses PCIe twice (the 12.8 MB channel buffer up, an image down).  The *_dev forms take
 * device pointers, queue their kernels on the context's stream and return without synchronising:
 *     pbrt_us_acquire_queue_dev(scene, ..., d_channel, tx)      queued (pbrt_us_acquire_dev: the same, and waits)
 *     [pbrt_us_apply_pulse_dev(ctx, ..., d_channel, d_rf)]       pulse_model = "gaussian" only
 *     pbrt_das_beamform_dev(ctx, &das, d_rf, d_tx, d_elem_x, d_x, d_z, d_bf)
 *     pbrt_envelope_dev(ctx, nx, nz, d_bf, d_env)
 *     pbrt_log_compress_dev(ctx, nx * nz, d_env, 60, d_img)
 *     pbrt_dev_download(ctx, img, d_img, nx * nz * 4)            the ONE copy to the host; waits for the stream
 * Same kernels, same results bit for bit as the host-pointer forms (which stage their arguments and call the same code). */
/* pbrt_us_acquire_dev without the wait: the acquisition is queued on the context's stream and the call returns; the channel
 * buffer is complete for whatever is queued behind it (the image-formation *_dev calls) and for the host after
 * pbrt_ctx_synchronize / pbrt_dev_download.  Its statistics -- and the error of a tripped traversal guard, PBRT_E_DEVICE --
 * arrive with the next call on the context that waits for the stream or starts other work (pbrt_get_stats, pbrt_ctx_synchronize,
 * pbrt_dev_download, the next acquisition or render ...): that call finishes the queued acquisition first and returns its error.
 * tx_delays (host, may be NULL) is filled before the call returns. */
int pbrt_us_acquire_queue_dev(pbrt_scene *scene, const pbrt_us_params *p, uint32_t seed, uint32_t paths_per_ray,
                              uint32_t path_offset, uint32_t norm_paths, void *d_channel_buf, float *tx_delays);

/* replaces: ultraspy DelayAndSum.beamform(d_data, scan) (USMain.py:204), data and tables in HBM.  All pointers are device
 * pointers: d_data [n_angles][n_elements][time_samples], d_tx_delays [n_angles][n_elements], d_elem_x [n_elements],
 * d_x [nx], d_z [nz], d_out [nx][nz]. */
int pbrt_das_beamform_dev(pbrt_ctx *ctx, const pbrt_das_params *p, const void *d_data, const void *d_tx_delays,
                          const void *d_elem_x, const void *d_x, const void *d_z, void *d_out);
/* The transmit half of the delays depends on the transmit delays and the scan grid only, and the reference's loop changes neither
 * (one probe, one GridScan, 51 renders: USMain.py:129-204): pbrt_das_first_arrival_dev writes the table
 *     d_table[a][ix][iz] (double) = t_tx(a; x, z) = min_e' (tx_delays[a][e'] + |(x, z) - (elem_x[e'], 0)| / c)
 * once, pbrt_das_beamform_table_dev beamforms with it: the same image bit for bit as pbrt_das_beamform_dev (which evaluates that
 * minimum per call), without the pass over all elements.  Both queue their kernel on the context's stream and return. */
int pbrt_das_first_arrival_dev(pbrt_ctx *ctx, const pbrt_das_params *p, const void *d_tx_delays, const void *d_elem_x,
                               const void *d_x, const void *d_z, void *d_table);
int pbrt_das_beamform_table_dev(pbrt_ctx *ctx, const pbrt_das_params *p, const void *d_data, const void *d_table,
                                const void *d_elem_x, const void *d_x, const void *d_z, void *d_out);
/* pbrt_das_beamform_probe in HBM: d_elem [n_elements][4], every other argument as in the three calls above; the table form is
 * bit-equal to the direct form here too. */
int pbrt_das_beamform_probe_dev(pbrt_ctx *ctx, const pbrt_das_params *p, const void *d_data, const void *d_tx_delays,
                                const void *d_elem, const void *d_x, const void *d_z, void *d_out);
int pbrt_das_first_arrival_probe_dev(pbrt_ctx *ctx, const pbrt_das_params *p, const void *d_tx_delays, const void *d_elem,
                                     const void *d_x, const void *d_z, void *d_table);
int pbrt_das_beamform_table_probe_dev(pbrt_ctx *ctx, const pbrt_das_params *p, const void *d_data, const void *d_table,
                                      const void *d_elem, const void *d_x, const void *d_z, void *d_out);
/* replaces: DelayAndSum.compute_envelope (USMain.py:205); d_rf, d_env [nx][nz], ranges that do not overlap (else PBRT_E_INVALID); NaN as pbrt_envelope */
int pbrt_envelope_dev(pbrt_ctx *ctx, uint32_t nx, uint32_t nz, const void *d_rf, void *d_env);
/* replaces: the log compression of USMain.py:210-218; d_env, d_out [n] (may be the same buffer); NaN as pbrt_log_compress */
int pbrt_log_compress_dev(pbrt_ctx *ctx, uint32_t n, const void *d_env, float dynamic_range_db, void *d_out);
/* the pulse model (RayTracingV0.py:194-204) on a channel buffer in HBM; d_in, d_out [n_traces][time_samples], not overlapping */
int pbrt_us_apply_pulse_dev(pbrt_ctx *ctx, uint32_t n_traces, uint32_t time_samples, float fs, float frequency, float sigma,
                            const void *d_in, void *d_out);

/* ---- p-DAS and F-DMAS beamformers, and the axial band-pass they need ------------------------------------------------
 * `ultraspy` ships PDelayAndSum and FilteredDelayMultiplyAndSum beside DelayAndSum; it is absent here (as for pbrt_das_beamform above),
 * so the arithmetic is this build's own definition, taken from the papers (Polichetti et al. 2018 for p-DAS, Matrone et al. 2015 for
 * F-DMAS).  s_e, the delayed sample of transmission a and element e at a pixel, is exactly the term pbrt_das_beamform adds (first
 * arrival, f64 position, range rules, f-number aperture of the line or of the element table, nearest / linear interpolation); U(a)
 * the elements the pixel uses for transmission a.  Per transmission
 *   PBRT_BF_PDAS:   r_e = sgn(s_e) |s_e|^(1/p),  q_a = sum_{e in U(a)} r_e,  y_a = sgn(q_a) |q_a|^p
 *                   (p = 2: sqrtf and a product; every other p: powf with the exponents 1.0f / p and p)
 *   PBRT_BF_FDMAS:  r_e = sgn(s_e) sqrt|s_e|,    y_a = sum_{i < j} r_i r_j, computed as ((sum_e r_e)^2 - sum_e |s_e|) / 2
 * and out = sum_a y_a, divided by n_angles when compound_mean is set; a pixel that uses no element is exactly 0.  All in f32: wave
 * w = e % 4 sums its share of sum r_e (and of sum |s_e|) per transmission, the four shares are added in wave order BEFORE the
 * non-linearity, the y_a in order of a.  Non-finite samples get no special treatment.  The F-DMAS output still holds its baseband
 * term: its band-pass around twice the carrier (and p-DAS's around the carrier) is pbrt_axial_fir, a separate step. */
#define PBRT_BF_PDAS 1u
#define PBRT_BF_FDMAS 2u
typedef struct pbrt_bf_params {
    pbrt_das_params das;
    uint32_t method; /* PBRT_BF_PDAS / PBRT_BF_FDMAS; anything else (0 included: plain DAS has its own calls) is PBRT_E_INVALID */
    float p;         /* PBRT_BF_PDAS: finite, 1 <= p <= 8, else PBRT_E_INVALID; not read for PBRT_BF_FDMAS */
    uint32_t probe;  /* 0: element positions [n_elements]; 1: the element table [n_elements][4] of pbrt_us_array_elements */
} pbrt_bf_params;
/* host pointers, arguments as pbrt_das_beamform / pbrt_das_beamform_probe; everything those refuse is refused here */
int pbrt_bf_beamform(pbrt_ctx *ctx, const pbrt_bf_params *p, const float *data, const float *tx_delays, const float *elem,
                     const float *x, const float *z, float *out);
/* device pointers, queued on the context's stream and recordable like pbrt_das_beamform_dev / pbrt_das_beamform_table_dev; the
 * table is pbrt_das_first_arrival_dev's (or its _probe twin's), and the table form is bit-equal to the direct form */
int pbrt_bf_beamform_dev(pbrt_ctx *ctx, const pbrt_bf_params *p, const void *d_data, const void *d_tx_delays, const void *d_elem,
                         const void *d_x, const void *d_z, void *d_out);
int pbrt_bf_beamform_table_dev(pbrt_ctx *ctx, const pbrt_bf_params *p, const void *d_data, const void *d_table, const void *d_elem,
                               const void *d_x, const void *d_z, void *d_out);
/* Axial FIR of an image [nx][nz]: out[ix][n] = sum_{k = -K .. K} taps[K + k] in[ix][n - k], samples outside the column zero, f32
 * multiply-adds in order of increasing k.  taps [2 K + 1] are the caller's (the library does not design them); K <= 1024 and
 * nz > 0 and in / out not overlapping, else PBRT_E_INVALID.  The _dev form takes device pointers (taps included), is queued and recordable. */
int pbrt_axial_fir(pbrt_ctx *ctx, uint32_t nx, uint32_t nz, uint32_t K, const float *taps, const float *in, float *out);
int pbrt_axial_fir_dev(pbrt_ctx *ctx, uint32_t nx, uint32_t nz, uint32_t K, const void *d_taps, const void *d_in, void *d_out);

/* ---- I/Q beamforming: demodulation, complex delay-and-sum, modulus envelope ---------------------------------------
 * The other half of ultraspy's users (`ultraspy.rf2iq`, `beamformer.set_is_iq(True)`, `compute_envelope` = the modulus; absent here as
 * above, so this is the build's own definition).  Complex samples and pixels are interleaved (re, im) float pairs.
 *
 * pbrt_rf2iq.  Sample j of a trace x[0 .. time_samples) was taken at t_j = t0 + j / fs.  Mixing: phi_j = frac(demod_freq * t_j),
 * evaluated in f64 and rounded to f32; u_j = x_j cospi(2 phi_j), v_j = -x_j sinpi(2 phi_j) in f32.  Low-pass and decimation by
 * D = decimation: for m in [0, Td), Td = ceil(time_samples / D),
 *   out[m] = 2 * ( sum_{k = -K .. K} taps[K + k] u[m D - k],  sum_k taps[K + k] v[m D - k] ),
 * samples outside the trace zero, f32 multiply-adds in order of increasing k, the factor 2 last.  Output sample m belongs to time
 * t0 + m D / fs.  in [n_traces][time_samples] floats, out [n_traces][Td] pairs, taps [2 K + 1] the caller's (as pbrt_axial_fir).
 * PBRT_E_INVALID for time_samples == 0, decimation outside [1, 8], K > 1024, fs not finite and > 0, t0 not finite, a non-finite or
 * negative demod_freq, and in / out overlapping.
 *
 * pbrt_iq_beamform.  data [n_angles][n_elements][time_samples] PAIRS at the rate das.fs (the I/Q rate), sample m at das.t0 + m / fs.
 * The delayed sample s_{a,e} of a pixel is what pbrt_das_beamform adds -- the same first arrival t_tx(a), f64 position, range
 * rules, f-number aperture of the line (probe = 0) or of the element table (probe = 1), nearest / linear interpolation (on both
 * components, with the one f32 weight) -- and is turned back by the carrier phase of its delay, split into a receive and a
 * transmit factor:
 *   rot_e = exp(i 2 pi frac(demod_freq * d_e / c)),   rot_a = exp(i 2 pi frac(demod_freq * t_tx(a)))
 *   (each frac in f64, rounded to f32, then sincospif of twice that),
 *   q_a = sum_{e in U(a)} rot_e * s_{a,e},   out = sum_a rot_a * q_a,   divided by n_angles when compound_mean is set.
 * A complex product (c, s) * (x, y) is (fmaf(c, x, -(s y)), fmaf(c, y, s x)) in f32.  Wave w = e % 4 sums its share of q_a per
 * transmission, the four shares are added in wave order, then rot_a is applied and the transmissions are added in order of a.  out
 * [nx][nz] pairs; a pixel that uses no element is exactly (0, 0).  demod_freq = 0 and zero imaginary parts give pbrt_das_beamform's
 * sums in another order.  Everything pbrt_das_beamform refuses is refused, and a non-finite or negative demod_freq, and probe > 1.
 *
 * pbrt_iq_envelope.  env[i] = sqrtf(fmaf(re, re, im * im)) for the n pixels of an image: no transform, so no limit on nz and no
 * column rule -- NaN and infinity propagate by this arithmetic, per pixel.  iq and env distinct.
 *
 * The _dev forms take device pointers (taps included), are queued on the context's stream and recordable like their RF neighbours;
 * the table of pbrt_iq_beamform_table_dev is pbrt_das_first_arrival_dev's (or its _probe twin's), bit-equal to the direct form. */
typedef struct pbrt_iq_params {
    pbrt_das_params das; /* das.fs: the rate of the I/Q data */
    float demod_freq;    /* Hz, finite and >= 0 */
    uint32_t probe;      /* 0: element positions [n_elements]; 1: the element table [n_elements][4] of pbrt_us_array_elements */
} pbrt_iq_params;
int pbrt_iq_beamform(pbrt_ctx *ctx, const pbrt_iq_params *p, const float *iq, const float *tx_delays, const float *elem,
                     const float *x, const float *z, float *out);
int pbrt_iq_beamform_dev(pbrt_ctx *ctx, const pbrt_iq_params *p, const void *d_iq, const void *d_tx_delays, const void *d_elem,
                         const void *d_x, const void *d_z, void *d_out);
int pbrt_iq_beamform_table_dev(pbrt_ctx *ctx, const pbrt_iq_params *p, const void *d_iq, const void *d_table, const void *d_elem,
                               const void *d_x, const void *d_z, void *d_out);
int pbrt_rf2iq(pbrt_ctx *ctx, uint32_t n_traces, uint32_t time_samples, float fs, float t0, float demod_freq, uint32_t decimation,
               uint32_t K, const float *taps, const float *in, float *out);
int pbrt_rf2iq_dev(pbrt_ctx *ctx, uint32_t n_traces, uint32_t time_samples, float fs, float t0, float demod_freq,
                   uint32_t decimation, uint32_t K, const void *d_taps, const void *d_in, void *d_out);
int pbrt_iq_envelope(pbrt_ctx *ctx, uint32_t n, const float *iq, float *env);
int pbrt_iq_envelope_dev(pbrt_ctx *ctx, uint32_t n, const void *d_iq, void *d_env);

/* ---- sector scans: beamforming on pixel tables, and scan conversion -------------------------------------------------
 * replaces: ultraspy's beamformers on a PolarScan (its beamformers take ravelled pixel lists; absent here as above, so this is the
 * build's own definition).  A scan is two tables px[n0][n1], pz[n0][n1] (float, axis 1 fastest, metres, in the probe's frame) instead
 * of the axes x[nx], z[nz]: das.nx = n0, das.nz = n1, and pixel (i0, i1) sits at ((double)px[i0 n1 + i1], (double)pz[i0 n1 + i1]).
 * Nothing else differs from the call the method names -- pbrt_das_beamform (PBRT_SCAN_DAS), pbrt_bf_beamform (PBRT_BF_PDAS,
 * PBRT_BF_FDMAS) or pbrt_iq_beamform (PBRT_SCAN_IQ): the same first arrival, f64 sample position, range rules, f-number aperture of
 * the line (probe = 0) or of the element table (probe = 1), interpolation, non-linearity or carrier rotation, and the same order of
 * the sums (wave w = e % 4, trips of angles, elements, angles; tiles of 8 x 8 over (i0, i1)).  On the tables of a separable scan,
 * px[i0][i1] = x[i0], pz[i0][i1] = z[i1], the result is that call's bit for bit.  out [n0][n1] floats, or (re, im) pairs for
 * PBRT_SCAN_IQ, whose data are pairs too; a pixel that uses no element is exactly 0.
 * One family carries the method and the probe flag in its parameter block.  Refused with PBRT_E_INVALID: everything pbrt_das_beamform
 * refuses, a method other than the four, probe > 1, PBRT_BF_PDAS with p not finite or outside [1, 8], PBRT_SCAN_IQ with demod_freq
 * not finite or negative (p is read by PBRT_BF_PDAS only, demod_freq by PBRT_SCAN_IQ only).
 * The _dev forms take device pointers, are queued on the context's stream and recordable like pbrt_das_beamform_dev;
 * pbrt_scan_first_arrival_dev writes d_table[a][i0][i1] (double) = min_e' (tx_delays[a][e'] + |pixel - element e'| / c), the statement
 * of pbrt_das_first_arrival_dev on the tables, and pbrt_scan_beamform_table_dev beamforms with it: bit-equal to the direct form. */
#define PBRT_SCAN_DAS 0u
#define PBRT_SCAN_IQ 3u
typedef struct pbrt_scan_params {
    pbrt_das_params das; /* das.nx = n0, das.nz = n1; das.fs: the rate of the data (PBRT_SCAN_IQ: of the I/Q data) */
    uint32_t method;     /* PBRT_SCAN_DAS, PBRT_BF_PDAS, PBRT_BF_FDMAS, PBRT_SCAN_IQ */
    float p;             /* PBRT_BF_PDAS: finite, 1 <= p <= 8 */
    float demod_freq;    /* PBRT_SCAN_IQ: Hz, finite and >= 0 */
    uint32_t probe;      /* 0: element positions [n_elements]; 1: the element table [n_elements][4] of pbrt_us_array_elements */
} pbrt_scan_params;
int pbrt_scan_beamform(pbrt_ctx *ctx, const pbrt_scan_params *p, const float *data, const float *tx_delays, const float *elem,
                       const float *px, const float *pz, float *out);
int pbrt_scan_beamform_dev(pbrt_ctx *ctx, const pbrt_scan_params *p, const void *d_data, const void *d_tx_delays, const void *d_elem,
                           const void *d_px, const void *d_pz, void *d_out);
int pbrt_scan_beamform_table_dev(pbrt_ctx *ctx, const pbrt_scan_params *p, const void *d_data, const void *d_table, const void *d_elem,
                                 const void *d_px, const void *d_pz, void *d_out);
int pbrt_scan_first_arrival_dev(pbrt_ctx *ctx, const pbrt_scan_params *p, const void *d_tx_delays, const void *d_elem,
                                const void *d_px, const void *d_pz, void *d_table);
/* replaces: the scan conversion a sector image needs before it is displayed (ultraspy users interpolate a PolarScan image onto a
 * grid with scipy).  src [n_theta][n_rho] (rho fastest) lies on the uniform axes theta_i = theta0 + i dtheta (radians, from the +z
 * axis towards +x) and rho_j = rho0 + j drho around the origin (ox, oz); dst [nx][nz] on the axes x[nx], z[nz].  Per output pixel,
 * in f64: dx = x - ox, dz = z - oz, rho = sqrt(dx dx + dz dz), theta = atan2(dx, dz), u = (theta - theta0) / dtheta,
 * v = (rho - rho0) / drho.  Inside iff 0 <= u <= n_theta - 1 and 0 <= v <= n_rho - 1; outside pixels are `fill` (any float, NaN
 * included).  Inside: i = min(floor(u), n_theta - 2), j = min(floor(v), n_rho - 2), the weights u - i and v - j rounded once to f32,
 * and three linear interpolations v0 + w (v1 - v0) (one fmaf each) in f32, in this order: along rho in row i, along rho in row i + 1,
 * then along theta.  Non-finite samples propagate through them and touch no pixel whose four corners do not hold them.
 * PBRT_E_INVALID for n_theta or n_rho < 2, nx or nz == 0, a non-finite theta0 / dtheta / rho0 / drho / ox / oz, and a zero step.
 * src and dst distinct.  The _dev form takes device pointers, is queued on the context's stream and recordable. */
typedef struct pbrt_scan_convert_params {
    uint32_t n_theta, n_rho, nx, nz;
    double theta0, dtheta, rho0, drho, ox, oz;
    float fill;
    uint32_t pad;
} pbrt_scan_convert_params;
int pbrt_scan_convert(pbrt_ctx *ctx, const pbrt_scan_convert_params *p, const float *src, const float *x, const float *z, float *dst);
int pbrt_scan_convert_dev(pbrt_ctx *ctx, const pbrt_scan_convert_params *p, const void *d_src, const void *d_x, const void *d_z,
                          void *d_dst);

/* ---- receive apodisation: a window on the f-number aperture of every beamformer -----------------------------------
 * replaces: ultraspy's DelayAndSum setups `rx_apodization` ('boxcar' / 'tukey') and `rx_apodization_alpha` (absent here as above, so
 * this is the build's own definition).  Every call above weighs the elements inside a pixel's f-number aperture with 1.  Here the
 * delayed sample s_{a,e} of a pixel whose element e lies inside the aperture is replaced by w_e * s_{a,e} (one f32 product; both
 * components of an I/Q sample, before rot_e) before anything else happens to it: delay-and-sum adds it, p-DAS and F-DMAS take the signed
 * root of the weighted sample (and F-DMAS' sum |s_e| is of weighted samples), I/Q turns it.  Nothing else differs from the call the
 * method names; the weight depends on the pixel and the element only, not on the transmission.
 *   u, the element's distance from the aperture's centre over the aperture's half width, in f64 from the doubles of the aperture test:
 *        line of elements:  u = |x - x_e| * (1 / (z / (2 f#)))     (one reciprocal per pixel)
 *        element table:     u = 2 f# |d_t| * (1 / d_n)             (one reciprocal per element)
 *   t = min(max((u - (1 - alpha)) * (1 / alpha), 0), 1) in f64 (alpha widened from its float; a NaN u -- z = 0 -- gives 0), rounded once to f32
 *   w = fmaf(1 - a0, cospif(t), a0) in f32, 1 - a0 one f32 subtraction
 *        PBRT_APOD_BOXCAR   w = 1: the kernels of the calls above, which hold no weight code -- the same image bit for bit
 *        PBRT_APOD_TUKEY    a0 = 1/2, alpha the caller's: 1 for u <= 1 - alpha, a raised cosine down to 0 at u = 1
 *        PBRT_APOD_HANN     a0 = 1/2, alpha = 1: Tukey(1), bit for bit
 *        PBRT_APOD_HAMMING  a0 = 0.54f, alpha = 1
 *   Error of a weight against its value in exact arithmetic: at most 4 * 2^-24 -- 2^-25 pi / 2 from rounding t (|dw/dt| <= pi / 2), 4 ulp
 *   of cospif on a value <= 1 times 1 - a0 <= 1/2, half an ulp of the fmaf (u and t in f64 add 1e-15 / alpha).
 * A weight of exactly 0 (Hann at u = 1) still multiplies: a non-finite sample there gives NaN.  A pixel that uses no element stays exactly
 * 0, the tiles no element sees are left as before, and the first-arrival table does not depend on the window: pbrt_das_first_arrival_dev
 * (tables = 0; _probe for scan.probe = 1) or pbrt_scan_first_arrival_dev (tables = 1) make it.
 * One block carries the whole request: scan keeps every rule of pbrt_scan_params (every method, probe), `tables` says whether the pixel
 * arguments are the axes x[nx], z[nz] or two pixel tables.  Refused with PBRT_E_INVALID besides: tables > 1, an unknown window,
 * PBRT_APOD_TUKEY with alpha not finite or outside (0, 1] (alpha is read by PBRT_APOD_TUKEY only), and a window other than boxcar with
 * das.f_number <= 0: there is no aperture to be a window of.  The three calls take the arguments of their pbrt_scan_* twins; the _dev forms
 * are queued on the context's stream and recordable, the table form is bit-equal to the direct form, and so is tables = 1 on the tables of
 * a separable scan to tables = 0. */
#define PBRT_APOD_BOXCAR 0u
#define PBRT_APOD_TUKEY 1u
#define PBRT_APOD_HANN 2u
#define PBRT_APOD_HAMMING 3u
typedef struct pbrt_apod_params {
    pbrt_scan_params scan; /* das, method (all four), p, demod_freq, probe: every rule of pbrt_scan_params */
    uint32_t tables;       /* 0: the axes x[nx], z[nz]; 1: two pixel tables [nx][nz] */
    uint32_t window;       /* PBRT_APOD_* */
    float alpha;           /* PBRT_APOD_TUKEY: finite, 0 < alpha <= 1 */
} pbrt_apod_params;
int pbrt_apod_beamform(pbrt_ctx *ctx, const pbrt_apod_params *p, const float *data, const float *tx_delays, const float *elem,
                       const float *px, const float *pz, float *out);
int pbrt_apod_beamform_dev(pbrt_ctx *ctx, const pbrt_apod_params *p, const void *d_data, const void *d_tx_delays, const void *d_elem,
                           const void *d_px, const void *d_pz, void *d_out);
int pbrt_apod_beamform_table_dev(pbrt_ctx *ctx, const pbrt_apod_params *p, const void *d_data, const void *d_table, const void *d_elem,
                                 const void *d_px, const void *d_pz, void *d_out);

/* ---- Capon: the minimum-variance beamformer on I/Q data --------------------------------------------------------------
 * replaces: ultraspy's Capon beamformer (absent here as above, so this is the build's own definition, after Synnevag, Austeng and Holm,
 * "Adaptive beamforming applied to medical ultrasound imaging", 2007, and "Benefits of minimum-variance beamforming in medical ultrasound
 * imaging", 2009).  Every call above weighs the elements by a rule fixed in advance; this one solves a small Hermitian system per pixel
 * and transmission.  data [n_angles][n_elements][time_samples] PAIRS, exactly as pbrt_iq_beamform takes them.  Per pixel and
 * transmission a, all in f32:
 *   U(a)   the elements pbrt_iq_beamform adds for that pixel and transmission -- the same first arrival, f64 position, range rules,
 *          f-number aperture of the line (probe = 0) or of the element table (probe = 1), nearest / linear interpolation -- taken in
 *          index order, N = |U(a)|
 *   v_k    (k = 0 .. N - 1) the delayed sample of the k-th element of U(a) turned by its receive rotation, v_k = rot_e * s_{a,e}, rot_e
 *          and the complex product as in pbrt_iq_beamform
 *   L = min(max(1, (uint32) floorf(l_prop * (float) N)), 32),  M = N - L + 1,  the subarrays x_l = (v_l .. v_{l+L-1}), l = 0 .. M - 1
 *   R = sum_l x_l x_l^H (L x L Hermitian, a sum and not a mean),  xbar = sum_l x_l,  tr = sum_i Re R_ii
 *   N == 0, or the comparison tr == 0 true:  y_a = (0, 0) exactly
 *   otherwise eps = delta_l * tr / (float) L, R' = R + eps I, u solves R' u = 1 by Cholesky (R' = G G^H, forward then backward
 *          substitution), y_a = ((float) N / (float) M) * (u^H xbar) / (sum_i Re u_i)
 *          -- in exact arithmetic N w^H mean_l(x_l) with w = R'^-1 1 / (1^H R'^-1 1).
 *   out = sum_a rot_a * y_a, rot_a as in pbrt_iq_beamform, added in order of a, divided by n_angles when compound_mean is set.
 * The scale of the data: y_a is homogeneous in the v_k, their squares are not.  Before the sums the v_k of a pixel and transmission are
 * multiplied by the power of two 2^(127 - e), e the biased exponent of max_k max(|Re v_k|, |Im v_k|) (a NaN is no maximum) clamped to
 * [1, 253], and y_a by 2^(e - 127) at the end: both exact, so no bit differs from the formulas above unless a square would have left the
 * range of f32 -- and data times a power of two give the image times that power, bit for bit.
 * The order of the sums as built (one wave per pixel and transmission, lanes share the entries):
 *   R_ij (i >= j) = sum over l ascending of v_{l+i} conj(v_{l+j}): re = fmaf(a.x, b.x, fmaf(a.y, b.y, re)), im = fmaf(a.y, b.x,
 *          fmaf(-a.x, b.y, im)); xbar_i = sum over l ascending; tr over i ascending; eps = delta_l * tr / L (product, then quotient)
 *   Cholesky by columns j ascending: t = R_ij (+ eps on the diagonal, added first) minus G_ik conj(G_jk) over k ascending, one fmaf per
 *          real product; G_jj = sqrtf(Re t), G_ij = t / G_jj (two f32 divisions)
 *   forward: t_i = 1 minus G_ik y_k over k ascending, y_i = t_i / G_ii; backward: t_i = y_i minus conj(G_ki) u_k over k DEscending,
 *          u_i = t_i / G_ii
 *   u^H xbar and sum Re u_i: the L terms (zeros up to 64) added as a butterfly (lane i with lane i ^ 32, ^ 16, .. ^ 1);
 *          y_a = (((float) N / (float) M) * num) / den per component
 * Non-finite samples get no special treatment: a pixel that reads one is non-finite in at least one component and no other pixel
 * changes by a bit.  A pixel that uses no element is exactly (0, 0), and the tiles no element of a line sees are left as before.
 * Facts that follow: L = 1 (l_prop = 0) gives y_a = sum_k v_k, pbrt_iq_beamform's image in another order of operations; if every v_k of
 * a pixel equals v then y_a = N v for every l_prop and delta_l.
 * `tables` says whether the pixel arguments are the axes x[nx], z[nz] or two pixel tables, as in pbrt_apod_params.  There is no receive
 * window: the method makes its own weights.  Refused with PBRT_E_INVALID: everything pbrt_scan_params refuses, scan.method !=
 * PBRT_SCAN_IQ, tables > 1, l_prop not finite or outside [0, 0.5], delta_l not finite, <= 0 or > 1e3, das.n_elements > 256.
 * pbrt_capon_beamform takes host pointers; the _dev forms take device pointers, are queued on the context's stream and recordable; the
 * table is the one pbrt_das_first_arrival[_probe]_dev / pbrt_scan_first_arrival_dev write, the table form is bit-equal to the direct
 * form, and so is tables = 1 on the tables of a separable scan to tables = 0. */
typedef struct pbrt_capon_params {
    pbrt_scan_params scan; /* das, method (PBRT_SCAN_IQ only), demod_freq, probe: every rule of pbrt_scan_params */
    uint32_t tables;       /* 0: the axes x[nx], z[nz]; 1: two pixel tables [nx][nz] */
    float l_prop;          /* subarray length over the aperture's element count: finite, 0 <= l_prop <= 0.5 */
    float delta_l;         /* diagonal loading over the mean diagonal entry of R: finite, 0 < delta_l <= 1e3 */
} pbrt_capon_params;
int pbrt_capon_beamform(pbrt_ctx *ctx, const pbrt_capon_params *p, const float *iq, const float *tx_delays, const float *elem,
                        const float *px, const float *pz, float *out);
int pbrt_capon_beamform_dev(pbrt_ctx *ctx, const pbrt_capon_params *p, const void *d_iq, const void *d_tx_delays, const void *d_elem,
                            const void *d_px, const void *d_pz, void *d_out);
int pbrt_capon_beamform_table_dev(pbrt_ctx *ctx, const pbrt_capon_params *p, const void *d_iq, const void *d_table, const void *d_elem,
                                  const void *d_px, const void *d_pz, void *d_out);

/* ---- spatial coherence: SLSC and the coherence factor on I/Q data ------------------------------------------------------
 * The calls above weigh or solve for AMPLITUDES; these two image the COHERENCE of the aperture.  `ultraspy` has neither, so this is the
 * build's own definition, after Lediju, Trahey, Byram and Dahl, "Short-lag spatial coherence of backscattered echoes", 2011 (SLSC) and
 * Mallart and Fink 1994 / Hollman, Rigby and O'Donnell 1999 (the coherence factor, CF).  data [n_angles][n_elements][time_samples] PAIRS
 * at the rate das.fs, demodulated at demod_freq, exactly as pbrt_iq_beamform takes them.  Per pixel and transmission a, all in f32:
 *   U(a)   the elements whose centre sample pbrt_iq_beamform would take -- the same first arrival, f64 position, aperture rule and range
 *          rule -- ranked k = 0 .. N - 1 in element order, as Capon ranks them
 *   s_k[h] (h = -H .. H, H = half_kernel, 0 <= H <= 4) the trace at the delayed position plus h whole samples, by the interpolation rule
 *          and with the SAME weight w as the centre.  Linear (i0 the whole part of the position, w its fraction): das_lerp(w, trace[i0 + h],
 *          trace[i0 + h + 1]) = fmaf(w, t1 - t0, t0) per component if 0 <= i0 + h < T - 1; trace[T - 1] if i0 + h == T - 1 and w == 0;
 *          (0, 0) otherwise.  Nearest (r the rounded position): trace[r + h] if 0 <= r + h <= T - 1, else (0, 0).
 *   v_k[h] = rot_e * s_k[h] with the centre's rot_e = exp(2 pi i frac(f_d d_e / c)) and the complex product as in pbrt_iq_beamform: v_k[0]
 *          is bit for bit the v_k of Capon and of pbrt_iq_beamform.
 * PBRT_COH_SLSC (half_kernel H, lag_prop): the image is FLOAT32 [nx][nz].
 *   1. every row v_k[.] is multiplied by the power of two 2^(127 - e), e the biased exponent of max_h max(|Re v_k[h]|, |Im v_k[h]|) (a
 *      NaN is no maximum) clamped to [1, 253]: exact, Capon's device for the aperture, here per row
 *   2. P_k = sum over h ascending of fmaf(re, re, fmaf(im, im, P))
 *   3. u_k[h] = v_k[h] / sqrtf(P_k) (one IEEE square root per row, an IEEE division per component); the row is all zeros when the
 *      comparison P_k == 0 is true
 *   4. C(i, j) = Re sum_h u_i[h] conj(u_j[h]): over h ascending, c = fmaf(a.x, b.x, fmaf(a.y, b.y, c))
 *   5. R_a(m) = (sum_{i = 0}^{N - m - 1} C(i, i + m)) / (N - m)
 *   6. M = min(max(1, (uint32) floorf(lag_prop * (float) N)), N - 1, 64); M = 0 for N < 2
 *   7. y_a = sum_{m = 1}^{M} R_a(m), over m ascending.  As built (one wave per pixel, lane l holds the ranks l, l + 64, ...): for a lag m
 *      a lane adds the C(i, i + m) of its ranks i ascending (those with i + m < N), the 64 lanes' sums meet in a butterfly (lane l with
 *      lane l ^ 32, ^ 16, .. ^ 1), and that sum is divided by (float)(N - m) (an IEEE division): traces that are +-1 give R_a(m) exactly
 *   8. out = clamp(sum_a y_a), added in order of a and divided by n_angles when compound_mean is set (before the clamp); clamp(v) is v if
 *      v > 0, v if v is NaN, else +0.  No rot_a is applied: it cancels.
 *   A pixel that uses no element is exactly +0.  SLSC is homogeneous of degree 0 in every trace: a trace times a power of two changes no bit.
 * PBRT_COH_CF (gamma; half_kernel must be 0): the image is COMPLEX [nx][nz] pairs.
 *   1. the v_k = v_k[0] of the aperture are brought to order 1 by ONE power of two (Capon's rule: e of the maximum over k), undone on S_a
 *   2. S_a = sum_k v_k, 3. Q_a = sum_k fmaf(re, re, fmaf(im, im, .)): a lane adds its ranks ascending, the lanes meet in the butterfly
 *   4. CF_a = |S_a|^2 / ((float) N * Q_a) with |S|^2 = fmaf(S.x, S.x, S.y * S.y); 0 when the comparison Q_a == 0 is true
 *   5. w_a = 1 when gamma == 0, CF_a when gamma == 1, powf(CF_a, gamma) otherwise
 *   6. out = sum_a rot_a * (w_a * S_a * 2^(e - 127)), rot_a as in pbrt_iq_beamform, in order of a, divided by n_angles for compound_mean.
 *      A transmission with N = 0 is skipped, as in Capon.
 *   With gamma = 0 it is pbrt_iq_beamform's image in another order of operations.  A pixel that uses no element is exactly (+0, +0).  CF
 *   is homogeneous of degree 1: data times a power of two give the image times that power, bit for bit.
 * Non-finite samples propagate as this arithmetic carries them.  `tables` as in pbrt_apod_params; there is no receive window.
 * Refused with PBRT_E_INVALID: everything pbrt_scan_params refuses, scan.method != PBRT_SCAN_IQ, tables > 1, a kind other than the two
 * (a zeroed block is refused), das.n_elements > 256; SLSC: lag_prop not finite or outside (0, 1], half_kernel > 4; CF: gamma not finite or
 * outside [0, 4], half_kernel != 0.  A refused call leaves `out` untouched.
 * `out` holds nx * nz floats (SLSC) or nx * nz pairs (CF); pbrt_coherence_beamform takes host pointers and stages the width that `kind`
 * implies; the _dev forms take device pointers, are queued on the context's stream and recordable; the table is the one
 * pbrt_das_first_arrival[_probe]_dev / pbrt_scan_first_arrival_dev write, the table form is bit-equal to the direct form, so is tables = 1
 * on the tables of a separable scan to tables = 0, and the host form to _dev. */
#define PBRT_COH_SLSC 1u
#define PBRT_COH_CF 2u
typedef struct pbrt_coherence_params {
    pbrt_scan_params scan; /* das, method (PBRT_SCAN_IQ only), demod_freq, probe: every rule of pbrt_scan_params */
    uint32_t tables;       /* 0: the axes x[nx], z[nz]; 1: two pixel tables [nx][nz] */
    uint32_t kind;         /* PBRT_COH_SLSC or PBRT_COH_CF */
    uint32_t half_kernel;  /* SLSC: H <= 4, the axial kernel is 2 H + 1 samples; CF: 0 */
    float lag_prop;        /* SLSC: the lags summed over the aperture's element count: finite, 0 < lag_prop <= 1 */
    float gamma;           /* CF: the exponent of the weight: finite, 0 <= gamma <= 4 */
} pbrt_coherence_params;
int pbrt_coherence_beamform(pbrt_ctx *ctx, const pbrt_coherence_params *p, const float *iq, const float *tx_delays, const float *elem,
                            const float *px, const float *pz, float *out);
int pbrt_coherence_beamform_dev(pbrt_ctx *ctx, const pbrt_coherence_params *p, const void *d_iq, const void *d_tx_delays,
                                const void *d_elem, const void *d_px, const void *d_pz, void *d_out);
int pbrt_coherence_beamform_table_dev(pbrt_ctx *ctx, const pbrt_coherence_params *p, const void *d_iq, const void *d_table,
                                      const void *d_elem, const void *d_px, const void *d_pz, void *d_out);

/* ---- non-finite and out-of-range geometry in the beamformers ---------------------------------------------------------
 * Covers pbrt_das_beamform*, pbrt_bf_*, pbrt_iq_beamform*, pbrt_apod_beamform*, pbrt_scan_beamform*, pbrt_capon_beamform*,
 * pbrt_coherence_beamform* (which behave as Capon does wherever Capon is named below: a transmission whose first arrival is +-inf or
 * 1e300 adds nothing because N = 0, a NaN table entry with linear interpolation gives a NaN pixel) and the
 * first-arrival table calls, in every form.  The tables that decide WHICH SAMPLE a pixel reads -- the transmit delays tx[a][e], the
 * element positions or the element table (x_e, z_e, nx_e, nz_e), the pixel axes or pixel tables, and a first-arrival table ttx[a][pixel]
 * handed to a _table_dev form -- are not checked by any call (in the _dev forms they live in device memory).  A NaN, an infinity or a
 * position beyond 2^31 samples in them is not an error.  What happens instead, from the code as built, the same in the host, _dev and
 * _table_dev forms bit for bit (tests/geom_util.py, tests/test_gpu_geometry_nonfinite.py):
 *   No read leaves a trace or a table, and no pixel other than those named below changes by a bit.
 *   First arrival.  t_tx(a; pixel) is the f64 minimum (fmin, which drops a NaN operand) over the elements whose tx[a][e] + d_e / c is not
 *     NaN, started from 1e300: a NaN or +inf delay or distance leaves the minimum to the other elements, a transmission without any such
 *     element has the first arrival 1e300 (so does its entry in a table the library makes), and a -inf delay makes it -inf.
 *   A term (a, e) is taken only if the aperture comparison holds and the position lies in the trace; both are comparisons, false for NaN.
 *     A line of elements: an element whose position is NaN or infinite receives nothing (|x - x_e| <= half width is false) and gives no
 *     first arrival.  A NaN position bounds nothing; an infinite one widens the span the tile test uses (tiles are left early only when
 *     no pixel's aperture reaches into [min x_e, max x_e], taken with fminf / fmaxf, which skip NaN), which costs time and changes no bit.
 *     An element table with f_number > 0: a row with a NaN in its position or in its normal receives nothing (d_n > 0 is false); with the
 *     position finite and only the normal NaN it still takes part in the first arrival.  With f_number <= 0 the normal is not read and every
 *     element receives every pixel: an element whose POSITION is NaN then has a NaN receive part -- nearest interpolation takes nothing;
 *     linear interpolation indexes the trace by the transmit part alone and, where that lies in the trace, takes a sample with a NaN
 *     weight: a NaN pixel.  (The one arm in which a bad element does not simply drop out.)
 *   A pixel whose x or z is NaN or infinite takes no term and is exactly (+0) [(+0, +0)] in every family; with axes that is the whole
 *     column or row.  So is a finite pixel so far away that its positions leave the trace (x = 3e5 m).
 *   Positions beyond 2^31 samples.  Nearest interpolation decides on the f64 sum (t_tx + d_e / c - t0) fs: rint, two comparisons with 0 and
 *     T - 1, then the conversion.  Linear interpolation keeps the two parts (t_tx - t0) fs and d_e fs as whole samples (int32, converted with
 *     saturation, NaN -> 0) plus an f32 fraction, adds the whole parts and the carry of the fractions in wrapping 32-bit arithmetic and
 *     compares the sum AS AN UNSIGNED number with T - 1.  The receive part is never negative (a square root times fs > 0).  With it in
 *     [0, 2^31) and the transmit part inside +-2^31 the result is the f64 rule's; a part at or beyond +-2^31 saturates and the sum is
 *     refused: 2^31 - 1 plus anything non-negative, and -2^31 plus anything up to 2^31 - 1, are >= 2^31 > T - 1 as unsigned numbers.  One
 *     corner remains: a finite transmit part at or below -2^31 AND a receive part at or above 2^31 - 1 whose f32 fractions carry sum to
 *     0 and read samples 0 and 1 -- inside the trace, not the f64 rule's (a pixel 10^5 m away under t0 = +100 s).  (das.t0 = -200 s at
 *     20 MHz: every position is beyond 2^31, every image exactly zero.)
 *   What a transmission with a non-finite first arrival (all delays NaN: 1e300; a -inf delay; a NaN or +-inf table entry) adds:
 *     delay-and-sum, p-DAS, F-DMAS, their windowed forms and Capon add nothing for +-inf and 1e300 (no position lies in the trace; Capon:
 *       N = 0), and the image is that of the other transmissions.  A NaN table entry: nearest interpolation takes nothing; linear
 *       interpolation indexes the trace by the receive part alone with a NaN weight -- a NaN pixel (Capon: both components) wherever an
 *       element of the aperture has floor(d_e fs) in [0, T - 2].
 *     I/Q and windowed I/Q (the walk): wave 0 turns the transmission's sum by rot_a = exp(2 pi i frac(f_d t_tx)) whether or not a term
 *       was taken.  For t_tx = 1e300 that is (1, 0) and the zero sum stays (+0, +0).  For t_tx = -inf, +inf or NaN it is NaN: the pixel is
 *       NaN in both components -- at EVERY pixel of every 8 x 8 tile that is walked, whether the pixel itself sees an element or not.  A
 *       line of elements: the tiles in which some pixel's aperture reaches into the span of the elements; the other tiles are left early
 *       with exact zeros.  An element table: every tile.  A table entry reaches its own pixel only.
 *       So "Capon with L = 1 is I/Q delay-and-sum" does not hold on such input: Capon skips the transmission (N = 0), the walk gives NaN.
 *   The same delays, elements and pixels give the same bits whether the first arrivals come from the walk's own pass or from
 *     pbrt_das_first_arrival*_dev / pbrt_scan_first_arrival_dev on the same tables. */

/* ---- colour and power Doppler on an ensemble of beamformed I/Q frames ----------------------------------------------
 * replaces: ultraspy's Doppler module (apply_wall_filter, get_color_doppler_map, get_power_doppler_map; absent here as above, so this
 * is the build's own definition, the lag-one autocorrelation estimator of Kasai et al. 1985).  frames [n_frames][nx][nz] are (re, im)
 * float pairs, each frame an image as pbrt_iq_beamform writes it; frame n is pulse n, at slow time n / prf.  Two steps, one block.
 *
 * pbrt_doppler_autocorr: frames and the wall-filter basis -> acf [3][nx][nz] floats, the planes Re R1, Im R1, R0.  Per pixel, with
 * x_n its sample in frame n, N = n_frames, all in f32:
 *   wall (clutter) filter, the polynomial regression filter of degree d = wall_degree: y = x - Q^T (Q x).  q [d + 1][N] floats is the
 *          caller's table, row k the k-th member of an orthonormal basis of the polynomials of degree <= d on the points 0 .. N - 1
 *          (the library does not make it; d = 0 is mean removal).  The ensemble is first referred to its first frame, u_n = x_n - x_0
 *          (one f32 subtraction per component): a constant lies in the span of every basis, so y does not change, but what does not
 *          move from pulse to pulse -- the clutter the filter is there for -- is gone before anything is summed, and N identical
 *          frames give y = 0, and so acf = 0, exactly.  Then the coefficients, each component by itself:
 *              c_k = sum over n ascending of q[k][n] * u_n          (c = fmaf(q[k][n], u_n, c), from 0)
 *          then, per frame, y_n = u_n minus q[k][n] * c_k over k ascending   (y = fmaf(-q[k][n], c_k, y), from u_n).
 *          PBRT_DOPPLER_WALL_NONE: y_n = x_n, and q is not read (it may be NULL).
 *   lag zero: r0 = sum over n ascending of |y_n|^2, r0 = fmaf(y.re, y.re, fmaf(y.im, y.im, r0)) from 0;  R0 = r0 / (float) N
 *   lag one:  R1 = sum over n = 1 .. N - 1 ascending of y_n conj(y_{n-1}), with a = y_n, b = y_{n-1}:
 *              re = fmaf(a.re, b.re, fmaf(a.im, b.im, re)),   im = fmaf(a.im, b.re, fmaf(-a.re, b.im, im)),   both from 0
 *   The frames are swept twice (coefficients, then filter and correlation), once with PBRT_DOPPLER_WALL_NONE.
 *
 * pbrt_doppler_maps: acf -> velocity [nx][nz] and amplitude [nx][nz].  Each plane of acf is smoothed by a separable window of kx x kz
 * pixels (both odd), hx = kx / 2, hz = kz / 2, pixels outside the image zero (a 'same' convolution), in f32:
 *   weights w[0 .. k) of a k-point window, in f64 and rounded once to f32: PBRT_DOPPLER_BOXCAR 1 / k; PBRT_DOPPLER_HAMMING
 *          h_i / (h_0 + h_1 + .. + h_{k-1}) (added in that order) with h_i = 0.54 - 0.46 cos(2 pi i / (k - 1)), and 1 for k = 1
 *   along z first: t[ix][iz] = sum over j = 0 .. kz - 1 ascending of wz[j] * a[ix][iz + j - hz]    (t = fmaf(wz[j], a, t), from -0.0f)
 *   then along x:  s[ix][iz] = sum over i = 0 .. kx - 1 ascending of wx[i] * t[ix + i - hx][iz],   rows outside the image zero
 *          Both sums start from -0.0f, not +0.0f: the first fmaf then gives the product itself, the sign of a zero included (+0.0f
 *          would turn a product of -0.0f into +0.0f), and pixels outside the image, which are +0.0f, still add up to +0.0f.
 *   velocity = (float) (nyquist_velocity / pi) * atan2f(s_Im, s_Re), the factor from the doubles, rounded once; a pixel whose smoothed
 *          R1 compares equal to (0, 0) has velocity exactly 0
 *   amplitude = sqrtf(s_R0): the root of a power, so that pbrt_log_compress of it is the power-Doppler display
 *          (20 log10 of an amplitude = 10 log10 of a power)
 *   A 1 x 1 window (weight 1) leaves every plane as it is, bit for bit, -0.0f included: amplitude = sqrtf(-0.0f) = -0.0f there.
 * Range and non-finite values: non-finite samples and acf values get no special treatment, and the arithmetic of both steps is plain
 * f32 without rescaling.  A NaN or an infinity in a pixel's ensemble makes all three acf planes of that pixel non-finite and touches
 * no other pixel; in an acf plane it reaches the kx x kz pixels whose window holds it, in the map that reads the plane (R1: velocity,
 * R0: amplitude) and in no other; atan2f of an infinite R1 is finite, sqrtf of a negative or -inf R0 is NaN.  A power of two on the
 * frames is the square of it on acf, bit for bit, the same velocity and that power of two on the amplitude, while no product leaves
 * the normal range of f32; products below that range lose bits or vanish, and such pixels read as zero motion and zero power.
 * Sign: pbrt_rf2iq mixes with exp(-i 2 pi f t) and the beamformer turns a pixel back by the phase of its own delay, so a target that
 * moves AWAY from the probe (its echo arrives later from pulse to pulse) gives a NEGATIVE velocity, one that moves towards it a
 * positive one: velocity = -v_z for nyquist_velocity = c prf / (4 f), |v_z| below it.
 * The frames must come from a pulse whose carrier moves with the target (pulse_model 'gaussian' of the acquisition); the 'impulse'
 * model ties the carrier to absolute time, and a moving target then shifts no phase.
 * Each step reads the fields named for it and holds only those to their rules.  PBRT_E_INVALID: a null pointer (q may be NULL with
 * PBRT_DOPPLER_WALL_NONE only); n_frames outside [2, 64]; wall_degree neither PBRT_DOPPLER_WALL_NONE nor <= 3, or wall_degree + 1 >=
 * n_frames; kx or kz even or outside [1, 15]; an unknown window; nyquist_velocity not finite or <= 0; n_frames * nx * nz, nx * nz or a
 * grid dimension outside 32 bits; input and output overlapping.  nx * nz == 0 does nothing.  The _dev forms take device pointers (q
 * included), are queued on the context's stream and recordable like their neighbours. */
#define PBRT_DOPPLER_WALL_NONE 0xffffffffu
#define PBRT_DOPPLER_BOXCAR 0u
#define PBRT_DOPPLER_HAMMING 1u
typedef struct pbrt_doppler_params {
    uint32_t n_frames, nx, nz; /* the ensemble [n_frames][nx][nz]; n_frames is read by pbrt_doppler_autocorr only */
    uint32_t wall_degree;      /* autocorr: 0 .. 3, or PBRT_DOPPLER_WALL_NONE */
    uint32_t kx, kz;           /* maps: the smoothing window in pixels, odd, 1 .. 15 */
    uint32_t window;           /* maps: PBRT_DOPPLER_BOXCAR / PBRT_DOPPLER_HAMMING */
    float nyquist_velocity;    /* maps: m/s, finite and > 0: the velocity of a phase step of pi between two pulses */
} pbrt_doppler_params;
int pbrt_doppler_autocorr(pbrt_ctx *ctx, const pbrt_doppler_params *p, const float *frames, const float *q, float *acf);
int pbrt_doppler_autocorr_dev(pbrt_ctx *ctx, const pbrt_doppler_params *p, const void *d_frames, const void *d_q, void *d_acf);
int pbrt_doppler_maps(pbrt_ctx *ctx, const pbrt_doppler_params *p, const float *acf, float *velocity, float *amplitude);
int pbrt_doppler_maps_dev(pbrt_ctx *ctx, const pbrt_doppler_params *p, const void *d_acf, void *d_velocity, void *d_amplitude);

/* waits for everything queued on the context's stream */
int pbrt_ctx_synchronize(pbrt_ctx *ctx);
/* Device buffers for a caller without a GPU library of its own (the reference's driver is NumPy: USMain.py:103-121).
 * pbrt_dev_upload copies in stream order (a pageable source is staged before it returns: the caller may reuse it at once);
 * pbrt_dev_download copies in stream order and waits; pbrt_dev_free waits for the stream first. */
int pbrt_dev_alloc(pbrt_ctx *ctx, uint64_t bytes, void **out);
int pbrt_dev_free(pbrt_ctx *ctx, void *p);
int pbrt_dev_upload(pbrt_ctx *ctx, void *dst_dev, const void *src_host, uint64_t bytes);
int pbrt_dev_download(pbrt_ctx *ctx, void *dst_host, const void *src_dev, uint64_t bytes);

/* Per-step device times of the image-formation entry points (host and *_dev forms alike), HIP events on the ctx stream.
 * Off by default (an event pair per step costs a few microseconds of queue time each); pbrt_ctx_set_profiling(ctx, 1) turns
 * them on, pbrt_get_image_stats waits for the stream and reports the most recent call of each step since then. */
typedef struct pbrt_image_stats {
    double pulse_ms, das_ms, envelope_ms, log_ms;
    uint64_t das_model_bytes; /* algorithmic bytes of the last DAS call: the channel buffer once + the image once */
    uint32_t measured;        /* bit 0 pulse, 1 das, 2 envelope, 3 log: steps that ran with profiling on */
    uint32_t pad;
} pbrt_image_stats;
int pbrt_ctx_set_profiling(pbrt_ctx *ctx, int on);
int pbrt_get_image_stats(pbrt_ctx *ctx, pbrt_image_stats *out);

/* The keep table of the LAST radiance render of the context (csrc/tile_cull.h; PBRT_FILM_NO_TILE_CULL), for tests and diagnosis:
 * whether that render walked its first bounce with one, the region of the film it was built for, and the words themselves --
 * word b, bit i: primitive i can be met by the camera rays of region indices [64 b, 64 b + 63].  n_blocks == 0: that render had no
 * table (a BVH scene, more than 32 primitives, a region whose pixel count is no multiple of 64, PBRT_FILM_NO_TILE_CULL), or the
 * context has not rendered yet; the region is then 0.  builds counts the launches of the kernel that fills the table since the
 * context was made: a render that repeats scene, camera and region leaves it alone.  Waits for the context's stream, then copies
 * min(n_blocks, capacity) words to `words` (may be NULL with capacity 0).  Refused while a recording is open. */
typedef struct pbrt_tile_keep_info {
    uint32_t n_blocks;         /* words of the table: rw * rh / 64, or 0 */
    uint32_t rx0, ry0, rw, rh; /* the rendered region in film pixels: the crop widened by the filter's reach, clipped to the film */
    uint32_t pad;
    uint64_t builds;
} pbrt_tile_keep_info;
int pbrt_ctx_tile_keep(pbrt_ctx *ctx, pbrt_tile_keep_info *info, uint32_t *words, uint32_t capacity);

/* ---- the queued chain as ONE submission (hipGraph) ---------------------------------------------------------------------
 * At the reference's own size (320 rays x 1 path, USMain.py:36) the chain above is eight small kernels, three fills and a copy:
 * the host spends as long queueing them as the device spends running them, 100 times per script.  Between
 * pbrt_ctx_record_begin and pbrt_ctx_record_end the queueing entry points (pbrt_us_acquire_queue_dev, pbrt_us_apply_pulse_dev,
 * pbrt_das_beamform_dev, pbrt_das_beamform_table_dev, pbrt_bf_beamform_dev, pbrt_bf_beamform_table_dev, pbrt_axial_fir_dev,
 * pbrt_rf2iq_dev, pbrt_iq_beamform_dev, pbrt_iq_beamform_table_dev, pbrt_iq_envelope_dev,
 * pbrt_scan_beamform_dev, pbrt_scan_beamform_table_dev, pbrt_scan_first_arrival_dev, pbrt_scan_convert_dev,
 * pbrt_apod_beamform_dev, pbrt_apod_beamform_table_dev, pbrt_capon_beamform_dev, pbrt_capon_beamform_table_dev,
 * pbrt_coherence_beamform_dev, pbrt_coherence_beamform_table_dev,
 * pbrt_doppler_autocorr_dev, pbrt_doppler_maps_dev, pbrt_envelope_dev, pbrt_log_compress_dev) are RECORDED on the context's
 * stream instead of run; pbrt_graph_launch replays the recording in one submission and returns without waiting, exactly as if
 * the recorded calls had just been made: same kernels, same arguments, same results bit for bit, the acquisition's statistics
 * arrive with the next call that waits (kernel_ms / bounce_ms are 0: a replay carries no event pairs).
 *  - Arguments are frozen at recording time: parameter blocks, seeds, path counts and every device pointer.  What the kernels
 *    READ through those pointers is not: pbrt_scene_update_material between two launches is seen by the second one (the
 *    finite-difference loop of USMain.py:262-289 changes one roughness per render and nothing else).
 *  - The workspace must be warm: run the chain once the ordinary way first; a recorded call that would have to allocate, or to
 *    upload a table, fails (PBRT_E_NOMEM / PBRT_E_INVALID; the message names the buffer or table).  An error of a recorded
 *    call leaves the recording open: close it with pbrt_ctx_record_end, which reports the error again and makes no graph.
 *    Any other entry point on the context is refused with PBRT_E_INVALID while a recording is open (the recording stays good).
 *  - A recording goes stale when the context frees or replaces memory it refers to (a larger request for the same workspace
 *    buffer, pbrt_ctx_trim, pbrt_dev_free, pbrt_scene_destroy) or uploads other acquisition tables: pbrt_graph_launch then
 *    returns PBRT_E_INVALID and launches nothing; record again. */
typedef struct pbrt_graph pbrt_graph;
int pbrt_ctx_record_begin(pbrt_ctx *ctx);
int pbrt_ctx_record_end(pbrt_ctx *ctx, pbrt_graph **out);
int pbrt_graph_launch(pbrt_graph *g);
/* waits for the context's stream (a replay may still run).  Destroy a context's recordings before the context. */
int pbrt_graph_destroy(pbrt_graph *g);

#ifdef __cplusplus
}
#endif
#endif /* PBRT_HIP_H */
