/*
 * tactile_gym_hip.h — C ABI of libtactile_gym_hip.so: the MI355X-native vectorised tactile-env step.
 *
 * The reference (ac-93/tactile_gym) has no FFI layer of its own: its hot path is Python calling the PyBullet C
 * extension.  This header is therefore the boundary a maintainer would bind *instead of* those PyBullet calls;
 * every entry point cites the reference call sites it replaces (paths relative to tactile_gym/).  All arguments
 * are plain pointers and sizes; no torch or HIP types appear in signatures (streams and device pointers travel as
 * `void*`).  Every function returns 0 on success or a negative error code; tg_last_error() gives the message
 * (the reference calls sys.exit(msg) on bad mode strings — base_tactile_env.py:264, robot.py:65,174 — the Python
 * host layer turns a non-zero status into an exception).
 *
 * Threading: one context per (process, GPU); calls on one context are not re-entrant (the reference is single
 * threaded per env with one PyBullet client per process, base_tactile_env.py:51,59).  tg_step() only enqueues work
 * on the context's stream; tg_sync() waits — they map to SB3's VecEnv.step_async()/step_wait().
 */
#ifndef TACTILE_GYM_HIP_H
#define TACTILE_GYM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TG_MAX_DOF 8
#define TG_MAX_BODIES_PER_LINK 4
#define TG_ABI_VERSION 16
#define TG_MAX_TRAJ_POINTS 16

/* ---- robot description: the flattened URDF (replaces loadURDF, robots/arms/robot.py:95-112) --------------------- */
typedef struct {
    int32_t ndof;
    int32_t topology;                       /* 0: serial chain (UR5), 1: MG400 tree {-1,0,1,2,3,0,5,6} */
    double joint_pos[TG_MAX_DOF][3];        /* joint origin in parent link frame */
    double joint_rot[TG_MAX_DOF][9];        /* joint frame in parent link frame, row-major */
    double joint_axis[TG_MAX_DOF][3];
    /* rigid bodies welded to each moving link (URDF links incl. fixed children); mass 0 = empty slot */
    double body_mass[TG_MAX_DOF][TG_MAX_BODIES_PER_LINK];
    double body_com[TG_MAX_DOF][TG_MAX_BODIES_PER_LINK][3];
    double body_rot[TG_MAX_DOF][TG_MAX_BODIES_PER_LINK][9];
    double body_inertia[TG_MAX_DOF][TG_MAX_BODIES_PER_LINK][3];
    /* frames the reference reads with getLinkState (PyBullet inertial-frame convention) */
    int32_t tcp_link;     double tcp_pos[3];    double tcp_rot[9];     /* base_robot_arm.py:136-151 */
    int32_t sensor_link;  double sensor_pos[3]; double sensor_rot[9];  /* tactile_sensor.py:153-155 */
    double gravity[3];                      /* base_tactile_env.py:126 */
    double linear_damping, angular_damping; /* base_robot_arm.py:24 */
    double joint_damping;                   /* base_robot_arm.py:25 */
    double max_force, pos_gain, vel_gain;   /* ur5.py:19-21, mg400.py:27-29 */
    double rest_q[TG_MAX_DOF];              /* rest_poses.py (movable joints) */
} tg_robot;

/* ---- tactile sensor: camera + reference images (sensors/tactile_sensor.py:63-80,127-187) ------------------------- */
typedef struct {
    int32_t image_h, image_w;
    double cam_pos[3];                      /* camera mount in the sensor-body frame */
    double cam_rpy[3];
    double fov_deg, near_plane, far_plane;
    int32_t turn_off_border;
    const float*   nodef_dep;               /* host pointers, [h*w]; copied at tg_create */
    const float*   nodef_gray;
    const uint8_t* border_mask;
} tg_sensor;

/* ---- stimulus mesh seen by the tactile camera (edge_follow_env.py:218-235 loadURDF of the edge) ------------------ */
typedef struct {
    int32_t n_verts, n_tris;
    const float*   verts;                   /* host, [n_verts][3], object frame */
    const int32_t* tris;                    /* host, [n_tris][3] */
} tg_mesh;

enum { TG_ENV_EDGE_FOLLOW = 0, TG_ENV_SURFACE_FOLLOW_AUTO = 1, TG_ENV_OBJECT_BALANCE = 2, TG_ENV_OBJECT_PUSH = 3, TG_ENV_OBJECT_ROLL = 4 };
enum { TG_MOVE_XY = 0, TG_MOVE_XYZ = 1, TG_MOVE_XYRZ = 2, TG_MOVE_XYZRZ = 3 };            /* edge_follow_env.py:345-369 */
enum { TG_SMOVE_YZ = 0, TG_SMOVE_XYZ = 1, TG_SMOVE_YZRX = 2, TG_SMOVE_XYZRXRY = 3, TG_SMOVE_XRZ = 4 };   /* surface_follow_auto_env.py:27-57; xRz: surface_follow_vert_env.py:29-48 */
enum { TG_BMOVE_XY = 0, TG_BMOVE_XYZ = 1, TG_BMOVE_RXRY = 2, TG_BMOVE_XYRXRY = 3 };         /* object_balance_env.py:398-424 */
enum { TG_PMOVE_Y = 0, TG_PMOVE_YRZ = 1, TG_PMOVE_XYRZ = 2, TG_PMOVE_TYRZ = 3, TG_PMOVE_TXTYRZ = 4 }; /* object_push_env.py:372-454 */
enum { TG_TRAJ_SIMPLEX = 0, TG_TRAJ_STRAIGHT = 1 };                                          /* object_push_env.py:248-313 */
enum { TG_NOISE_FIXED_HEIGHT = 0, TG_NOISE_RAND_HEIGHT = 1 };                               /* edge_follow noise_mode */
enum { TG_SNOISE_SIMPLEX = 0, TG_SNOISE_NONE = 1, TG_SNOISE_RANDOM = 2, TG_SNOISE_VERTICAL_SIMPLEX = 3 };                   /* surface_follow noise_mode (base_surface_env.py:448-471) */
enum { TG_REWARD_DENSE = 0, TG_REWARD_SPARSE = 1 };
enum { TG_PHYSICS_F64 = 0, TG_PHYSICS_F32 = 1 };
enum { TG_CONTACT_MAP_AUTO = 0, TG_CONTACT_MAP_LANE = 1, TG_CONTACT_MAP_WAVE = 2 };
enum { TG_CONTROL_TCP_VELOCITY = 0, TG_CONTROL_TCP_POSITION = 1 };                             /* robot.py:156-186 apply_action */

/* ---- task + engine configuration (env ctor kwargs / env_modes, edge_follow_env.py:23-134) ------------------------- */
typedef struct {
    int32_t abi_version;                    /* TG_ABI_VERSION */
    int32_t env_kind;                       /* TG_ENV_* */
    int32_t num_envs;
    int32_t max_steps;                      /* episode length cap */
    int32_t movement_mode, noise_mode, reward_mode;
    int32_t physics_dtype;                  /* TG_PHYSICS_* */
    int32_t action_repeat;                  /* sim ticks per env step: 24 (edge_follow_env.py:35-37) */
    int32_t solver_iterations;              /* 150 (base_tactile_env.py:128-130) */
    int32_t auto_reset;                     /* VecEnv semantics: reset finished envs inside tg_step */
    int32_t device;                         /* HIP device ordinal */
    double sim_dt;                          /* 1/240 */
    double min_action, max_action;          /* edge_follow_env.py:140 */
    double act_lo[6], act_hi[6];            /* per-dimension physical ranges, :143-166 */
    double tcp_lims[6][2];                  /* :75-90 */
    double workframe_pos[3], workframe_rpy[3]; /* :106-107 */
    double stim_pos[3];                     /* edge_pos :201 */
    double edge_height, edge_len;           /* :203-207 */
    double termination_dist;                /* :67 */
    double embed_dist, embed_lo, embed_hi;  /* :94-99, :291-298 */
    /* surface_follow (base_surface_env.py:234-282): heightfield stimulus generated per episode from OpenSimplex noise.
     * stim_pos = surface_pos; rows x cols grid of pitch surf_grid_scale; height = noise2(i*interp, j*interp) * range. */
    int32_t surf_rows, surf_cols;           /* 64, 64 (:240-243) */
    int32_t surf_center_z;                  /* 1: Bullet's heightfield shape is centred on (min+max)/2 [PARITY_ASSUMPTIONS A15] */
    int32_t pgs_full_sweeps;                /* 0 (default): the motor-row PGS leaves the loop once no impulse can change in its last bit
                                             * (Bullet's zero-residual exit, PARITY_ASSUMPTIONS A7b); 1: always run solver_iterations sweeps */
    double surf_grid_scale;                 /* 0.006 (:238) */
    double surf_height_range;               /* 0.025 (:239) */
    double surf_interp;                     /* 0.05  (:244) */
    double surf_xy_extent;                  /* 0.15  (:245) goal distance and TCP xy limits */
    double auto_action_scale;               /* 1.0 tactip / 0.9 digitac / 0.7 digit (surface_follow_auto_env.py:33-41) */
    /* object_balance (object_balance_env.py): a free rigid body (stimulus mesh = its visual triangles, in the body's base
     * inertial frame) tied to the TCP link by a point-to-point constraint. embed_lo/hi: rand_embed_dist range (:308-316). */
    int32_t rand_gravity, rand_embed;       /* env_modes flags (:39-41) */
    double gravity_lo, gravity_hi, gravity_default;   /* U(-1.0, -0.1) or -0.1 (:301-306) */
    double obj_mass;
    double obj_com[3];                      /* composite centre of mass in the base inertial frame */
    double obj_inertia[9];                  /* about obj_com, base axes, row major */
    double obj_root_inertial_pos[3];        /* root link's inertial origin in its link frame (loadURDF places the link frame) */
    double obj_base_width, obj_base_height; /* 0.1, 0.0025 (:158-159) */
    double obj_init_rpy[3];                 /* (0, 0, -pi/2) (:190) */
    double ext_force[3];                    /* apply_random_force_base: (0, 0, -0.1) (:360-381) */
    double term_deg, term_pos;              /* 35 deg, 0.1 m (:50-51) */
    double p2p_erp, p2p_max_impulse;        /* 0.2, 500 [PARITY_ASSUMPTIONS A18-A19] */
    /* object_push (object_push_env.py): a free cube (obj_mass / obj_com / obj_inertia, stimulus mesh = its visual triangles)
     * on the table, pushed by the collision core of the sensor tip along a per-episode trajectory of goals.
     * termination_dist = termination_pos_dist (:57); obj_init_rpy = (-pi, 0, pi/2) (:158). */
    int32_t traj_type;                      /* TG_TRAJ_* (env_modes["traj_type"]) */
    int32_t traj_n_points;                  /* 10 (:229), <= TG_MAX_TRAJ_POINTS */
    int32_t rand_init_orn, rand_obj_mass;   /* env_modes flags (:168-192) */
    int32_t tip_link, n_tip_verts;          /* moving link carrying the tip's collision core; its convex-hull vertices */
    int32_t cone_friction;                  /* enableConeFriction=1 (base_tactile_env.py:128-130) */
    int32_t surf_goal_variant;              /* surface_follow: 0 = -v0 auto-drive (surface_follow_auto_env.py), 1 = -v1: every action dimension from the
                                             * agent, dense reward -(goal_xy + 10 surf + w_norm cos) (surface_follow_goal_env.py:27-90) */
    const double* tip_verts;                /* host, [n_tip_verts][3], link frame; copied at tg_create */
    double obj_half[3];                     /* cube half extents 0.04 (:45-46) */
    double obj_init_pos[3];                 /* (:160) */
    double table_z;                         /* top of the table: 0 */
    double mu_table, mu_tip;                /* combined friction: cube 0.065 x table 1.0 / x tip lateral friction (:50-56, :216-225) */
    double margin_cube, margin_tip;         /* collision margins [PARITY_ASSUMPTIONS A24] */
    double contact_breaking, contact_erp;   /* 1e-4 [A24], 0.2 */
    double tip_stiffness, tip_damping;      /* contactStiffness / contactDamping of the tip core (:50-56) */
    double obj_lin_damp, obj_ang_damp;      /* Bullet defaults 0.04 */
    double traj_spacing, traj_max_perturb, traj_init_offset;   /* 0.025, 0.1, obj_width/2 + spacing (:229-262) */
    double mass_lo, mass_hi;                /* rand_obj_mass U(0.4, 0.8) (:190-192) */
    double init_orn_range, traj_ang_range;  /* pi/32 (:170), pi/8 (:283) */
    /* control mode (env_modes["control_mode"], robot.py:156-186).  TG_CONTROL_TCP_POSITION: the action is a work-frame pose delta
     * (act_lo/hi = +-1 mm, +-1 deg, e.g. edge_follow_env.py:143-153); target = clip(current + delta, tcp_lims), inverse kinematics,
     * POSITION_CONTROL motors (base_robot_arm.py:228-279, mg400.py:131-190), then blocking_move(max_steps = max_blocking_steps,
     * constant_vel = None) (robot.py:188-260). */
    int32_t control_mode;                   /* TG_CONTROL_* */
    int32_t max_blocking_steps;             /* _max_blocking_pos_move_steps = 10 (edge_follow_env.py:38) */
    /* object_push: goal index right after reset.  reset() ends with get_step_data() (base_object_env.py:183-185), whose termination()
     * advances the goal when the cube is within termination_pos_dist of it (:520-537); the first goal sits exactly that far from the
     * cube's start position, so whether index 0 or 1 comes out is decided by double rounding of the work-frame constants.  The host
     * evaluates that comparison once, the way the reference would (PARITY_ASSUMPTIONS A29). */
    int32_t reset_goal_id;
    /* surface_follow-v2 (noise_mode vertical_simplex, movement xRz; the `vertical_simplex` branches of base_surface_env.py and
     * surface_follow_vert_env.py): the heightfield stands upright, rotated by rpy (0, -pi/2, 0) about stim_pos = surface_pos
     * (x, y, 0.15 + range); the bins, the goal and the reward follow the reference's flipped surface_array (:476-516, :735-758);
     * reward -(10 surf_dist + 3 cos_dist) (surface_follow_vert_env.py:66-81). */
    int32_t surf_vertical;
    /* object_roll (object_roll_env.py): a marble (sphere.urdf: obj_mass, roll_radius; stimulus mesh = its tessellation at that radius)
     * on the table under the flat TacTip, whose tip collides as a URDF cylinder; goal given in the TCP frame.  Shares with object_push:
     * obj_mass, mu_table, mu_tip, contact_breaking / erp, tip_stiffness / damping, obj_lin / ang_damp, tip_link, cone_friction, table_z,
     * termination_dist (:60).  workframe_pos z = 2 roll_radius - embed_dist is the default; per episode it is 2 r - embed with
     * r = roll_radius x U(1, 2) (rand_obj_size) and embed = U(embed_lo, embed_hi) (rand_embed) (:181-201).  Movement "xy" only.
     * State view: obj_mass = the episode's radius, goal_pos = the goal in the TCP frame. [PARITY_ASSUMPTIONS A30] */
    int32_t roll_rand_init_pos, roll_rand_size, roll_rand_embed;   /* env_modes flags (:41-43) */
    double roll_radius;                     /* default_obj_radius 0.0025 (:161) */
    double roll_init_range;                 /* 0.009 (:210-214) */
    double roll_goal_lo, roll_goal_hi;      /* goal distance U(0.005 | 0 with rand_init_pos, 0.015) (:256-259) */
    double tip_cyl_pos[3], tip_cyl_rot[9];  /* tip cylinder frame (axis z) in the frame of tip_link */
    double tip_cyl_half_len, tip_cyl_radius;
    /* object_push / object_roll: how the contact solve of stepSimulation (robot.py:141; 150 PGS sweeps, base_tactile_env.py:127-130) is
     * mapped onto the GPU.  TG_CONTACT_MAP_WAVE: one 64-lane wavefront per env, one solver row per lane (fills the chip at ~1024 envs);
     * TG_CONTACT_MAP_LANE: one lane per env (fewer instructions per env, better once every SIMD is busy); AUTO picks by num_envs.
     * Same solver, same row order; results agree to rounding (f64), contact sets exactly.  The wave kernels are built for f64 with cone
     * friction (object_roll: the UR5; a tip hull that fits LDS); tg_create decides once per context, and any other combination steps AND resets
     * on the lane mapping whatever this field asks for (tg_get_step_mode: envs_per_wavefront 64). */
    int32_t contact_mapping;                /* TG_CONTACT_MAP_* */
    /* edge_follow / surface_follow with auto_reset: the reset of these envs (edge_follow_env.py:311-336, base_surface_env.py:616-662,
     * robot.py:114-125) is a pure function of the env's RNG stream, so every env's NEXT post-reset state is computed ahead of time on a
     * second low-priority stream ("reset bank") and a finished env takes it inside the step instead of stalling the batch for its blocking
     * move.  Results are identical with the bank on, off, or not ready in time (the same reset code either way) - for edge_follow and
     * surface_follow.  object_balance has a reset TEMPLATE instead (the arm's post-reset state computed once, by env 0's first reset): against
     * TG_BANK_OFF, which recomputes every reset with the fallen object still on the constraint, the arm differs by the last-bit residue of that
     * tick's Gauss-Seidel (joints within 1e-13 rad, frames within 3 pixels: tests/test_gpu_reset_bank.py) - not bit-identical.
     * TG_BANK_AUTO = TG_BANK_ON (round 5; until then on for the MG400 only - its blocking move stalls a 1024-env batch for 9-11 ms per
     * full-batch reset, 0.126 -> 1.13 M env-steps/s on surface_follow-v2).  The UR5's reset is 0.1 ms: nothing when every env finishes in the
     * same step (a random rollout from a common start), but with episodes ending in different steps - any RL run - some env finishes in nearly
     * every step and the whole batch waits for it each time: 6.7 -> 18.3 M env-steps/s at 1024 envs (tools/desync_rate.py); the aligned
     * rollout costs the same either way.  With the bank on, a context's step calls keep the host at most ~70 steps ahead of the device (the
     * refill's pacing: one host-side wait for a marker every 8 steps).  TG_BANK_OFF: every reset on the spot; TG_BANK_SYNC: on, and the refill
     * is waited for after every step (tests: the bank is always ready).  The environment variable TG_RESET_BANK (0 / 1 / sync) overrides. */
    int32_t reset_bank;                     /* TG_BANK_* */
    /* object_push: narrowphase of the tip-cube pair (stepSimulation's collision detection, robot.py:141).  TG_NARROW_CLOSED_FORM: the
     * deepest point of the tip's convex hull against the cube's faces in closed form, ONE contact point per tick (PARITY A24);
     * TG_NARROW_GJK_MANIFOLD: support-mapping GJK distance + EPA penetration on the hull and the box, fed into a persistent manifold of up
     * to 4 points with Bullet's add / replace / break rules (PARITY A35-A38); TG_NARROW_GJK_SINGLE: the same GJK / EPA, the tick's point only
     * (no cache): the closed form's special case - equal to it wherever the closest features are a hull vertex and a box face (tests).
     * Both run on the wave mapping (f64, cone friction). */
    int32_t narrowphase;                    /* TG_NARROW_* */
    /* object_balance, object_mode "ball_on_plate" (object_balance_env.py:187-199, 241-260): the free body is the round plate (obj_mass /
     * obj_com / obj_inertia, obj_base_width 0.2, tied to the TCP as the pole is) and a ball rolls on it: sphere.urdf x globalScaling 7.5
     * (mass 0.05 unscaled, radius 0.0025 x 7.5), lateralFriction 10 x the plate's default 0.5, reset to workframe + (0, 0, radius) with a
     * one-shot torque 0.001 x (U(-1,1), U(-1,1), 0) (:350-353, 393-401).  Contact: ball against the plate's solid cylinder (plate_radius,
     * half length obj_base_height / 2), contact_breaking / contact_erp / obj_lin_damp / obj_ang_damp as for object_push, cone friction.
     * Reward, termination and the observations ignore the ball (:426-497).  Lane mapping only.  [PARITY_ASSUMPTIONS A39] */
    int32_t balance_object;                 /* TG_BALANCE_* */
    double ball_radius, ball_mass, ball_mu, plate_radius;
    /* edge_follow, TCP_velocity_control, f64, 128-multiple images: the env step as ONE launch (csrc/tg_fused.hip) - the wavefront that steps an
     * env (base_tactile_env.py:166-185: apply_action .. get_observation is one chain per env) also resets it when its episode ended and draws
     * its tactile image(s) - instead of the three dependent launches k_step -> k_reset -> render.  Same step / reset code, the block raster's
     * arithmetic on another lane mapping: images, rewards, dones byte-identical, joint angles to the last bits (tests/test_gpu_fused_step.py).
     * Measured SLOWER on an MI355X (56 against 43 us per step at 1024 envs), hence TG_FUSED_AUTO = off; TG_FUSED_ON opts in;
     * the environment variable TG_FUSED_STEP (0 / 1) overrides.  tg_get_step_mode reports what runs. */
    int32_t fused_step;                     /* TG_FUSED_* */
    /* btContactSolverInfo::m_leastSquaresResidualThreshold of stepSimulation() (robot.py:141).  The reference's setPhysicsEngineParameter
     * call (base_tactile_env.py:127-130) passes fixedTimeStep, numSolverIterations, enableConeFriction and contactBreakingThreshold - NOT
     * solverResidualThreshold, so whatever PyBullet's physics server installs applies (PARITY_ASSUMPTIONS A7b: believed to be 1e-7; Bullet's
     * own library default is 0).  0 (default): the Gauss-Seidel loop leaves only at last-bit convergence, every mode of this library that
     * rests on that (the licensed analytic fixed point, the composed sweeps, object_balance's reset template) is available.  > 0 ("threshold
     * mode"): Bullet's rule - the loop leaves after the sweep whose largest squared row velocity change deltaImpulse / jacDiagABInv (a cone
     * friction pair counts once, with the sum of its two; A7c) is <= this, never before the first sweep, at most solver_iterations - evaluated
     * per env after every sweep on every mapping; every tick is a full tick, no licence, no composed sweeps, no reset template
     * (tg_state_view.solver_sweeps reports the sweeps run).  pgs_full_sweeps is ignored in this mode.  (ABI v13) */
    double solver_residual_threshold;
    /* object_balance, object_mode "spinning_plate" (balance_object = TG_BALANCE_SPINNING_PLATE; object_balance_env.py:107-108, 198-239, 267-269,
     * 355-358; ABI v14): the body on the TCP's constraint is the spool (plate_buffer.urdf: obj_mass / obj_com / obj_inertia describe IT, the
     * stimulus mesh is its mesh, its pivot sits at (0, 0, -spin_buffer_height / 2 + embed_dist) and is never updated) and the env's object - what
     * termination, reward and the oracle observation look at - is the dish (spinning_plate.urdf: spin_dish_*) standing on the spool's spindle.
     * Both collide as the convex hull of their mesh (margin spin_hull_margin each): the pair goes through the wave-mapped GJK / EPA and a
     * persistent manifold of up to four points (csrc/tg_spin.hip, PARITY_ASSUMPTIONS A35-A38, A41), friction spin_mu under the cone,
     * contact_breaking / contact_erp as for the other contact envs; the spool keeps obj_lin_damp / obj_ang_damp, the dish has none (:338-345).
     * Reset: dish to init_obj_pos = workframe + (0, 0, spin_buffer_height + obj_base_height / 2 - embed) - without the buffer height when
     * rand_embed is on, as upstream's reset_task (:317-321) -, spool to workframe + (0, 0, spin_buffer_height / 2), a one-tick torque (0, 0, -1)
     * in the dish's frame and ext_force at a random point of the dish (:355-358).  f64, UR5 chain, one wavefront per env; not with
     * solver_residual_threshold > 0.  Hull arrays are copied at tg_create. */
    double spin_dish_mass, spin_dish_com[3], spin_dish_inertia[9];
    double spin_buffer_height, spin_hull_margin, spin_mu;
    int32_t spin_n_dish, spin_n_spool;      /* hull vertex counts: n_dish <= 1152, n_spool <= 256 */
    const double* spin_dish_hull;           /* [spin_n_dish][3] in the dish's base frame */
    const double* spin_spool_hull;          /* [spin_n_spool][3] in the spool's base frame */
} tg_config;

enum { TG_BANK_AUTO = 0, TG_BANK_OFF = 1, TG_BANK_SYNC = 2, TG_BANK_ON = 3 };
enum { TG_NARROW_CLOSED_FORM = 0, TG_NARROW_GJK_MANIFOLD = 1, TG_NARROW_GJK_SINGLE = 2 };
enum { TG_BALANCE_POLE = 0, TG_BALANCE_BALL_ON_PLATE = 1, TG_BALANCE_SPINNING_PLATE = 2 };
enum { TG_FUSED_AUTO = 0, TG_FUSED_OFF = 1, TG_FUSED_ON = 2 };

typedef struct tg_ctx tg_ctx;

const char* tg_last_error(void);
int tg_abi_version(void);

/* gym.make(...) / env ctor: uploads constants, allocates per-env SoA state for num_envs envs, seeds env i with i. */
int tg_create(const tg_config* cfg, const tg_robot* robot, const tg_sensor* sensor, const tg_mesh* stimulus, tg_ctx** out);
int tg_destroy(tg_ctx* ctx);                                  /* env.close(), base_tactile_env.py:69-74 */

/* Use an existing HIP stream (e.g. torch's current stream) for all work; NULL = the context's own stream. */
int tg_set_stream(tg_ctx* ctx, void* hip_stream);

/* env.seed(s): per-env 64-bit seeds (SB3 convention seed+i), base_tactile_env.py:61-64. */
int tg_seed(tg_ctx* ctx, const uint64_t* seeds, int32_t n);

/* env.reset() for the envs whose mask byte is non-zero (NULL = all): task randomisation, rest pose, IK,
 * blocking move, first observation.  edge_follow_env.py:311-336, robot.py:114-125,188-260. Asynchronous. */
int tg_reset(tg_ctx* ctx, const uint8_t* host_mask);

/* env.step(a): actions float32[num_envs][act_dim] (device pointer if on_device, else host). Asynchronous.
 * base_tactile_env.py:166-185 -> robot.py:156-186 -> 24 x robot.py:131-141 -> tactile_sensor.py:261-294. */
int tg_step(tg_ctx* ctx, const float* actions, int32_t on_device);

int tg_sync(tg_ctx* ctx);                                     /* VecEnv.step_wait(): wait for enqueued work */

/* Device-resident results of the last step/reset (valid after tg_sync or on the context's stream).
 * The tactile observation buffer is READ-ONLY for the caller: for the edge / cube stimuli a render launch rewrites only the 16 x 16 pixel blocks
 * whose content changes (those it draws, and those an earlier launch drew that now show the untouched sensor again), so bytes a caller wrote into
 * it would survive into later observations.  TG_RASTER_REWRITE_ALL=1 in the environment makes every launch rewrite every block. */
int tg_get_obs_tactile(tg_ctx* ctx, void** dev_ptr);           /* uint8 [num_envs][H][W][1] */
int tg_get_terminal_obs(tg_ctx* ctx, void** dev_ptr);          /* uint8 [num_envs][H][W][1], rows valid where done */
int tg_get_reward_done_dev(tg_ctx* ctx, void** reward_f32, void** done_u8);
/* The three per-step outputs live in ONE device allocation: [tactile obs u8[N*H*W] | pad to 16 B | reward f32[N] | done u8[N]]
 * (tg_get_obs_tactile / tg_get_reward_done_dev point into it).  A rank ships this byte range to rank 0 as one message per step
 * (replaces SubprocVecEnv's per-env pickled pipes, sb3_helpers/rl_utils.py:17-30).  obs_bytes = offset of the reward. */
int tg_get_packed_outputs(tg_ctx* ctx, void** dev_ptr, int64_t* obs_bytes, int64_t* total_bytes);
/* Interior-only tactile payload for that message: the border ring of an image is a constant paste of the reference image
 * (tactile_sensor.py:291-292; 40 % of a 128 x 128 TacTip image), so a rank may ship only the 4-pixel words that hold a pixel inside the border
 * mask; *k = bytes per image (a multiple of 16; the pad repeats the last word).
 * tg_pack_interior: this context's current observations -> dst uint8 [num_envs][k] (device).  tg_unpack_interior (on the receiver; the
 * context only supplies the sensor constants): src uint8 [n_images][k] -> dst uint8 [n_images][H*W] with the ring restored.  Both are
 * enqueued on the context's stream.  *k = -1 with turn_off_border (the ring then carries rendered values). */
int tg_get_interior_count(tg_ctx* ctx, int32_t* k);
/* Reset bank (tg_config.reset_bank): how many auto-resets so far took a precomputed entry (*swapped) and how many were done on the spot because
 * the entry was not ready (*late); *mode = 0 bank off, 1 on, 2 on and waited for.  object_push (round 6): *mode = 3 - resets that took the reset
 * TEMPLATE (the arm's post-reset state is a function of constants while the tip stays clear of the previous episode's cube) / resets that ran their
 * blocking move; 0 with the template off.  Synchronises the context's stream. */
int tg_get_bank_stats(tg_ctx* ctx, int64_t* swapped, int64_t* late, int32_t* mode);
/* Render targets (multi-GPU; replaces the copy of rank 0's own observations into the gathered batch that SubprocVecEnv's parent does
 * per env, sb3_helpers/rl_utils.py:17-30): tg_set_obs_targets names up to two caller-owned device buffers uint8 [num_envs][H][W] - rank 0's
 * blocks of its two alternating gathered batches - and tg_select_obs_target picks where the NEXT steps / resets draw the tactile observations:
 * 0 = the context's own buffer (tg_get_packed_outputs), 1 / 2 = the caller's.  Each target has its own changed-block record (the block raster
 * rewrites only what changes, so a buffer must see every launch that is meant for it... or none).  Reward /
 * done / feature stay in the context's packed block; tg_get_obs_tactile returns the selected target.  count = 0 forgets the targets. */
int tg_set_obs_targets(tg_ctx* ctx, int32_t count, void* const* dev_ptrs);
int tg_select_obs_target(tg_ctx* ctx, int32_t index);
/* How tg_step runs on this context: *mode = 1 one launch per step (tg_config.fused_step; csrc/tg_fused.hip), 0 separate step / reset / render
 * launches; *envs_per_wavefront = envs one wavefront steps and draws in the one-launch form; in the separate form, envs one wavefront of the
 * context's step kernel steps (16: k_step_quad, a quad of lanes per env; 64: a lane per env; 1: a wavefront per env).  The step kernel is chosen
 * once, by tg_create, from tg_config, the robot and the stimulus: the answer is the same before and after the first step. */
int tg_get_step_mode(tg_ctx* ctx, int32_t* mode, int32_t* envs_per_wavefront);
int tg_pack_interior(tg_ctx* ctx, void* dst_dev);
int tg_unpack_interior(tg_ctx* ctx, const void* src_dev, int32_t n_images, void* dst_dev);
/* ---- tile-sparse tactile payload and direct stores into rank 0's memory (csrc/tg_exchange.hip) ------------------------------------
 * A tactile image is zero away from the contact patch and a constant paste on the border ring (tactile_sensor.py:261-294).  Cut into
 * 16 x 16 tiles, only the tiles that differ from that constant template travel (lossless; 9 % of the bytes of an edge_follow batch, 22 % of
 * object_balance at 256 x 256, 48 % surface_follow, 73 % object_push).  Message: one 16-byte header {u32 count, n_images, tiles per image,
 * magic} and `count` records of 272 bytes {u32 tile id = image * tiles_per_image + tile, 12 bytes pad, 16 rows x 16 pixels}; records are in
 * no particular order.  A reader tolerates what no pack kernel writes: a header whose magic or tiles per image is not its own is no message
 * (the template everywhere), a count above n_images * tiles_per_image is clamped to that, and a record whose id is not below
 * n_images * tiles_per_image - compared as unsigned 32-bit numbers - is ignored (with a list of previous ids the id is still recorded there,
 * and ignored again by the restore).  These entry points are context free (raw device pointers + a HIP stream; NULL = the default stream).
 * obs_dev, template_dev, src_dev and dst_dev of the tile entries are read and written 16 bytes at a time: each must be 16-byte aligned
 * (src_stride a multiple of 16 keeps every rank's message so); a pointer that is not is refused with -1, like a NULL one, before any launch.
 * tg_get_tile_template: the template of a context's sensor, uint8 [H][W] (device).
 * tg_pack_tiles: obs uint8 [n_images][h][w] -> dst (tg_tiles_capacity bytes; may be another GPU's memory opened with tg_ipc_open);
 *   counters_dev = two zeroed uint32 in LOCAL device memory (left zero again by every launch); tail_src_dev (may be NULL): tail_bytes (<= 1 MiB)
 *   copied to dst_dev + tail_offset by the same launch - the small block that rides behind the images (reward | done | feature).
 * tg_unpack_tiles: src message -> dst uint8 [n_images][h][w]: the template everywhere, then the records. */
int tg_get_tile_template(tg_ctx* ctx, void** dev_ptr);
int tg_tiles_capacity(int32_t n_images, int32_t h, int32_t w, int64_t* bytes);
int tg_pack_tiles(void* hip_stream, const void* obs_dev, const void* template_dev, int32_t n_images, int32_t h, int32_t w, void* dst_dev,
                  void* counters_dev, const void* tail_src_dev, int64_t tail_bytes, int64_t tail_offset);
int tg_unpack_tiles(void* hip_stream, const void* src_dev, const void* template_dev, int32_t n_images, int32_t h, int32_t w, void* dst_dev);
/* The same for the messages of n_ranks ranks in two launches: message r at src_dev + r * src_stride (bytes, a multiple of 16) ->
 * dst uint8 [n_ranks][n_images][h][w]; rank skip_rank (-1: none) is left alone (rank 0 copies its own images instead of packing them).
 * prev_ids_dev (may be NULL = fill everything): uint32 [n_ranks][1 + n_images * tiles] zeroed by the caller, owned by this destination
 * buffer: the list of tiles its last message had live; with it only those tiles get the template back before the new records land (dst
 * must hold the template to begin with). */
int tg_unpack_tiles_multi(void* hip_stream, const void* src_dev, int64_t src_stride, int32_t n_ranks, int32_t skip_rank, const void* template_dev,
                          int32_t n_images, int32_t h, int32_t w, void* dst_dev, void* prev_ids_dev);
/* Receive slots that peers store into directly (one process per GPU; the reference's counterpart is the pipe of each SubprocVecEnv worker,
 * sb3_helpers/rl_utils.py:17-30).  tg_ipc_alloc: zeroed device memory on the current device + its 64-byte IPC handle; tg_ipc_open /
 * tg_ipc_close: map / unmap it in another process (its GPU then reaches the memory over xGMI).  HSA_ENABLE_IPC_MODE_LEGACY=0 is required. */
int tg_ipc_alloc(int64_t bytes, void** dev_ptr, uint8_t* handle64);
int tg_ipc_alloc_was_uncached(void);   /* 1: the last tg_ipc_alloc of this process got uncached device memory; 0: the runtime refused and it is plain hipMalloc memory */
int tg_ipc_free(void* dev_ptr);
int tg_ipc_open(const uint8_t* handle64, void** dev_ptr);
int tg_ipc_close(void* dev_ptr);
/* Device copy on a stream whose destination (or source) may be memory opened with tg_ipc_open; both pointers 16-byte aligned. */
int tg_copy_bytes(void* hip_stream, void* dst_dev, const void* src_dev, int64_t bytes);
int tg_copy_bytes2(void* hip_stream, void* dst1_dev, const void* src1_dev, int64_t bytes1, void* dst2_dev, const void* src2_dev, int64_t bytes2);   /* two ranges, one launch */
/* tg_copy_bytes2 whose launch also raises n_flags flags (flags_dev[i * stride_words] = value, system-scope release; NULL: none). */
int tg_copy_bytes2_flag(void* stream, void* dst1_dev, const void* src1_dev, int64_t bytes1, void* dst2_dev, const void* src2_dev, int64_t bytes2,
                        void* flags_dev, int32_t n_flags, int32_t stride_words, uint32_t value);
/* Stream-ordered flags (uint32, monotone step counters) in such memory.  tg_flag_set: after everything enqueued before it on the stream has
 * finished, flags[i * stride_words] = value for i < n (release, system scope).  tg_flag_wait: the stream goes on once every
 * flags[i * stride_words] has reached value (compared modulo 2^32); after timeout_ms of waiting it goes on anyway and ORs bit (i & 31) into
 * *err_dev (uint32 in local device memory, may be NULL); a wait that finds *err_dev already non-zero goes on at once (one timeout has shown the
 * exchange to be broken: the later waits must not sit theirs out as well).  n <= 64. */
int tg_flag_set(void* hip_stream, void* flags_dev, int32_t n, int32_t stride_words, uint32_t value);
int tg_flag_wait(void* hip_stream, const void* flags_dev, int32_t n, int32_t stride_words, uint32_t value, void* err_dev, int32_t timeout_ms);
/* Envs with an "extended_feature" observation (object_push, object_roll) append it to the same allocation, so that config 4's
 * tactile_and_feature observation still travels as one message: [... | done u8[N] | pad to 4 B | feature f32[N][dim]]
 * (object_push_env.py:611-629).  *feature_off = byte offset of the feature block (-1: this env has none). */
int tg_get_packed_feature(tg_ctx* ctx, int64_t* feature_off, int32_t* dim);
/* "extended_feature" observation (object_push_env.py:611-629): float32 [num_envs][*dim]: TCP pos, rpy and current goal
 * pos, rpy in the work frame; terminal != 0: the copy taken at the last step (rows valid where done). */
int tg_get_obs_feature(tg_ctx* ctx, void** dev_ptr, int32_t* dim, int32_t terminal);
/* observation_mode "oracle" (get_oracle_obs: edge_follow_env.py:454-476, base_surface_env.py:789-819, object_balance_env.py:528-563,
 * object_push_env.py:571-609, object_roll_env.py:367-407): float32 [num_envs][*dim] computed on the device from the current state
 * (dim 10 / 20 / 26 / 30 / 34 by env kind).  Enqueued on the context's stream; the pointer stays valid for the context's lifetime. */
int tg_get_obs_oracle(tg_ctx* ctx, void** dev_ptr, int32_t* dim);
int tg_copy_obs_oracle(tg_ctx* ctx, float* host_dst);          /* synchronises */
/* observation_mode "oracle" as a per-step output: tg_step / tg_reset then also write the vectors (tg_get_obs_oracle returns them without a
 * launch of its own), and the step's own vectors - taken before the auto-reset - are kept: rows of the envs that finished are their
 * terminal observation (VecEnv info["terminal_observation"]).  Call before the first tg_step. */
int tg_enable_oracle_obs(tg_ctx* ctx);
int tg_get_obs_oracle_terminal(tg_ctx* ctx, void** dev_ptr);   /* float32 [num_envs][dim] */
int tg_copy_obs_oracle_terminal(tg_ctx* ctx, float* host_dst); /* synchronises */
/* Per-env episode statistics: what the reference's callers read from the Monitor wrapper they put around every env
 * (sb3_helpers/rl_utils.py:17-30, 59: info["episode"] = {"r", "l", "t"}).  The step kernels add up, in double, the float32 rewards they hand
 * out; when an env reports done its return and length (in env steps) are kept here until its next episode ends.  Rows valid where done. */
int tg_get_episode_stats(tg_ctx* ctx, void** final_return_f32, void** final_len_i32);      /* device: float32 [num_envs], int32 [num_envs] */
int tg_copy_episode_stats(tg_ctx* ctx, float* final_return, int32_t* final_len);           /* synchronises */
/* Host copies (synchronise). */
int tg_get_reward_done(tg_ctx* ctx, float* reward, uint8_t* done);
int tg_copy_obs_tactile(tg_ctx* ctx, uint8_t* host_dst, int32_t terminal);
/* The images of `count` chosen envs only: env_ids[k]'s tactile image (visual != 0: its scene-camera image, after tg_set_scene) goes to
 * host_dst + k * image_bytes, from the current observation buffer or (terminal != 0) from the terminal one.  What a VecEnv's step_wait reads
 * for info["terminal_observation"] (stable_baselines3's VecEnv contract; sb3_helpers/rl_utils.py:17-37 wraps the envs in one): with the
 * episodes out of phase a handful of envs finish in nearly every step, and copying the whole terminal batch for them (16.8 MB at 1024 x
 * 128 x 128) was two thirds of the numpy step's time.  ABI v12. */
int tg_copy_obs_rows(tg_ctx* ctx, int32_t visual, int32_t terminal, const int32_t* env_ids, int32_t count, uint8_t* host_dst);
/* The same for the envs that finished in the last step, without the host naming them (ABI v13, round 6): ONE launch on the context's stream compacts
 * the done flags and stores, straight into device-visible pinned host memory `dst_pinned` (tg_done_rows_bytes(cap) bytes, 16-byte aligned), a 16-byte
 * header {u32 count = envs done, u32 cap, u32 num_envs, u32 magic 0x74674452}, then int32 ids[cap] (ascending), float32 episode returns[cap], int32
 * episode lengths[cap] (the Monitor statistics of tg_get_episode_stats), then, 16-byte aligned, uint8 rows[cap][H * W]: the TERMINAL tactile images of
 * the first min(count, cap) finished envs.  What info["terminal_observation"] / info["episode"] need arrives under the synchronisation the
 * observation fetch makes anyway (sb3_helpers/rl_utils.py:17-37: SubprocVecEnv's workers send obs, reward, done and info in one message).
 * count > cap: the caller falls back to tg_copy_obs_rows / tg_copy_episode_stats for that step. */
int tg_done_rows_bytes(tg_ctx* ctx, int32_t cap, int64_t* bytes);
int tg_pack_done_rows(tg_ctx* ctx, void* dst_pinned, int32_t cap);
int tg_copy_obs_feature(tg_ctx* ctx, float* host_dst, int32_t terminal);   /* float32 [num_envs][12] */

/* Parity / inspection view of the per-env state, host arrays sized by the caller ([num_envs][...]), any may be NULL. */
typedef struct {
    double*  q;              /* [num_envs][ndof] */
    double*  qd;             /* [num_envs][ndof] */
    double*  qd_target;      /* [num_envs][ndof] joint velocity targets of the last controller call */
    double*  tcp_pos;        /* [num_envs][3] world, inertial-frame convention */
    double*  tcp_rpy;        /* [num_envs][3] */
    double*  edge_ang;       /* [num_envs] */
    double*  embed_dist;     /* [num_envs] */
    float*   stim_xform;     /* [num_envs][12] camera<-stimulus transform used by the last render */
    int32_t* step_count;     /* [num_envs] */
    int32_t* reset_ticks;    /* [num_envs] sim ticks used by the last reset's blocking move */
    uint64_t* rng_state;     /* [num_envs] */
    double*  goal_pos;       /* [num_envs][3] world (surface_follow) */
    double*  direction;      /* [num_envs][2] work-frame auto-drive direction (surface_follow) */
    double*  heights;        /* [num_envs][rows*cols] heightfield_data[row][col] (surface_follow) */
    float*   surf_zoff;      /* [num_envs] vertical centring offset applied to the rendered heightfield */
    double*  body_pos;       /* [num_envs][3] free object base frame (object_balance) */
    double*  body_rot;       /* [num_envs][9] row major */
    double*  body_linvel;    /* [num_envs][3] velocity of the composite centre of mass */
    double*  body_angvel;    /* [num_envs][3] */
    double*  gravity_z;      /* [num_envs] */
    double*  traj;           /* [num_envs][3][TG_MAX_TRAJ_POINTS] work-frame x, y, yaw of the goal trajectory (object_push) */
    int32_t* goal_id;        /* [num_envs] targ_traj_list_id (object_push) */
    double*  obj_mass;       /* [num_envs] (object_push) */
    /* Contact pairs of the last stepSimulation tick (robot.py:141), in solver row order (object_push / object_roll; 0 elsewhere:
     * the other envs filter every sensor contact out, tactile_sensor.py:46-57, base_surface_env.py:432).  An id names the pair by its
     * feature: 0-7 = cube vertex (index 4 ix + 2 iy + iz of the +-half extents) against the table, the marble's table contact is 0;
     * 8 + k = hull vertex k of the sensor tip's collision core against the cube (8 for the marble against the tip's cylinder).
     * Unused slots are -1.  Integer data: compared bit-exactly with the oracle. */
    int32_t* contact_count;  /* [num_envs] */
    int32_t* contact_ids;    /* [num_envs][8]: solver row order, -1 beyond contact_count (4 table + up to 4 tip slots) */
    double*  ball_pos;       /* [num_envs][3] object_balance ball_on_plate: the ball's centre, world */
    double*  ball_linvel;    /* [num_envs][3] */
    double*  ball_angvel;    /* [num_envs][3] */
    double*  ball_impulse;   /* [num_envs] normal impulse of the ball - plate contact in the last sim tick (0: not touching) */
    double*  dish_state;     /* [num_envs][20] spinning_plate: the dish's base position (0-2), orientation (3-11, row major), linear (12-14) and angular
                                (15-17) velocity, the last tick's summed normal impulse (18) and number of manifold points (19); body_* is the spool */
    int32_t* broadphase_pairs;  /* [num_envs] last broadphase check (tg_set_broadphase): unexpected pairs whose world AABBs overlap (stage 1) */
    int32_t* broadphase_hits;   /* [num_envs] ... of which the oriented boxes / the hull also overlap (stages 2, 3): 0 = no unmodelled contact possible */
    int32_t* broadphase_mask;   /* [num_envs] bit k: slot k is part of a hit */
    int32_t* solver_sweeps;  /* [num_envs] threshold mode (tg_config.solver_residual_threshold > 0): PGS sweeps the sim ticks of the env's last
                              * tg_step ran, summed over the ticks (a reset's ticks are not counted); zeros otherwise.  (ABI v13) */
} tg_state_view;
int tg_get_state(tg_ctx* ctx, const tg_state_view* view);
/* Overwrite joint state (tests): q, qd [num_envs][ndof]; re-evaluates the cached TCP pose. */
int tg_set_joint_state(tg_ctx* ctx, const double* q, const double* qd);
/* Inspection (tests): int32 [num_envs], the env steps for which each env's step may still take the analytic fixed point qd = target,
 * q += dt target without a new full solve.  0: the env's next step starts with a full solve; 8: the last step's full
 * solve converged within 80 % of the sweep budget; 7 .. 1: steps since then; a reset renews it or leaves 0, tg_set_joint_state leaves 0.
 * The arm steps take the shortcut only when every env of the wavefront holds a positive value (64 envs, 16 on the quad mapping,
 * tg_get_step_mode; the env's own on object_balance's wave mapping) AND the a-priori bound on the motor impulses holds in the tick.
 * Always 0 for the MG400, in threshold mode and on the kernels that solve every tick.  Synchronises.  A function added, no struct changed:
 * TG_ABI_VERSION stays. */
int tg_copy_step_licence(tg_ctx* ctx, int32_t* host_dst);

/* Per-kernel timing (bench.py's roofline leg).  enable = 1: HIP event pairs around every launch class on the launch stream, between the step's
 * launches; every figure carries what an EMPTY event pair measures (3 - 5 us).  enable = 2: only the kernels' own clock
 * (csrc/tg_kt.hpp: every wavefront stamps its start and end, wall_clock64; first start -> last end per class), no host call between the step's
 * launches - the figures of the rollout itself.  enable = 0: off.
 * tg_profile_get which: 0 step kernel, 1 render of all envs (the one launch of a fused step), 2 reset sequence, 3 masked render (reset /
 * auto-reset envs only), 4 scene camera, 5 an empty event pair - by HIP events; 8 + k (k = 0 .. 3): class k by the kernels' own clock. */
int tg_profile_enable(tg_ctx* ctx, int32_t enable);
int tg_profile_get(tg_ctx* ctx, int32_t which, double* total_ms, int64_t* launches);

/* ---- scene camera: the "visual" / "visuotactile" observations and render() (base_tactile_env.py:212-245, 284-320) -------------------
 * get_visual_obs draws the whole scene (plane, table, robot, stimulus) from a fixed world camera with getCameraImage and keeps rgb.
 * The triangle set is shared by all envs; each triangle is rigid in one frame: 0 the world, 1 + i moving link i (tg_robot numbering),
 * ndof + 1 the task's stimulus / free body (same frame as tg_mesh).  Upstream's pixels depend on the GL driver: PARITY_ASSUMPTIONS A31-A33. */
typedef struct {
    int32_t image_h, image_w;               /* rgb_image_size (= image_size upstream); <= 128 or a multiple of 128 */
    int32_t n_verts, n_tris;
    const float*   verts;                   /* host [n_verts][3] */
    const int32_t* tris;                    /* host [n_tris][3] */
    const uint8_t* tri_frame;               /* host [n_tris] */
    const uint8_t* tri_rgb;                 /* host [n_tris][3], the <material> colour */
    double cam_target[3], cam_dist, cam_yaw_deg, cam_pitch_deg;   /* rgb_cam_pos / _dist / _yaw / _pitch, e.g. edge_follow_env.py:176-195 */
    double fov_deg, near_plane, far_plane;  /* rgb_fov / rgb_near_val / rgb_far_val */
    double light_dir[3];                    /* world, towards the light */
    uint8_t background[3];
    uint8_t body_rgb[3];                    /* surface envs: colour of the per-env heightfield (changeVisualShape rgbaColor, base_surface_env.py:431) */
    int32_t body_heightfield;               /* != 0: the task's body is the env's heightfield (frame ndof + 1), not part of the triangle set */
    int32_t every_step;                     /* != 0: tg_step / tg_reset also draw the scene (observation modes with "visual" / "visuo") */
} tg_scene;
/* Uploads the scene; call before the first tg_step. */
int tg_set_scene(tg_ctx* ctx, const tg_scene* scene);

/* ---- broadphase guard (ABI v13; csrc/tg_broadphase.hip, oracle/broadphase.py) --------------------------------------------------------------------
 * PyBullet's stepSimulation (robots/arms/robot.py:141) runs Bullet's broadphase over the world AABBs of every collision object and hands every
 * overlapping pair of different bodies (not both static, neither filtered out) to the narrowphase.  This library's contact sets are FIXED per env
 * from the reference's collision filters (sensors/tactile_sensor.py:46-57, robots/arms/mg400/mg400.py:68-72, base_surface_env.py:432,
 * object_push_env.py:249): the guard checks per env step that no OTHER pair can touch - one oriented box per URDF link with <collision> geometry
 * (the robot's, the table, the plane, the stimulus, the free objects), world AABBs sorted and swept on x in the env's wavefront (stage 1: what
 * Bullet's broadphase would report), the pairs found narrowed by an oriented-box separating-axis test (stage 2) and, for a robot link against the
 * table, by the world extents of the link's convex hull (every vertex; grown by hull_margin + margin) against the table's margin box (stage 3).  Two
 * shapes within 2 * margin of each other at a check are always reported: every shape lies inside its box.  Results per env in tg_state_view.broadphase_pairs / _hits / _mask; a
 * non-zero hit count means PyBullet may generate a contact this library has no solver row for.
 * Slots: 0-15 the robot's boxes in URDF link order, 16 table, 17 plane, 18 edge stimulus, 19 / 20 the object's boxes, 21 the ball of
 * ball_on_plate.  src: where a slot's pose comes from - TG_BP_LINK the robot's moving link `link` (-1: the fixed base), TG_BP_WORLD none (center is
 * in the world), TG_BP_EDGE the episode's edge (stim_pos, yaw = edge angle), TG_BP_BODY the free body's pose, TG_BP_SPHERE its position only with the
 * box scaled to the episode's radius (object_roll), TG_BP_BALL the ball of ball_on_plate. */
enum { TG_BP_NONE = 0, TG_BP_LINK = 1, TG_BP_WORLD = 2, TG_BP_EDGE = 3, TG_BP_BODY = 4, TG_BP_SPHERE = 5, TG_BP_BALL = 6 };
#define TG_BP_SLOTS 22
typedef struct {
    double center[3], rot[9], half[3];      /* the box in the frame `src` names */
    int32_t src;                            /* TG_BP_* (TG_BP_NONE: empty slot, or a link the reference filters out) */
    int32_t link;                           /* TG_BP_LINK: moving link index, -1 = base */
    int32_t body;                           /* boxes of one body are never paired */
    int32_t is_static;                      /* two static boxes are never paired (robot base, table, plane, edge) */
    int32_t hull_off, hull_n;               /* TG_BP_LINK: the link's convex-hull vertices (moving-link frame) in `hull_verts`, for stage 3 */
    uint32_t expected;                      /* bit k: the pair (this slot, slot k) is one the solver has rows for */
    int32_t conj;                           /* -1, or the slot of a second box bounding the SAME shape (a disc: its square and the square turned 45
                                             * degrees): a pair with this slot is a hit only if the other box overlaps the second one as well */
} tg_bp_box;
typedef struct {
    tg_bp_box box[TG_BP_SLOTS];
    double margin;                          /* added to every half extent: shapes within 2 * margin at a check are reported (what that covers inside a step) */
    double hull_margin;                     /* Bullet inflates a URDF convex hull by gUrdfDefaultCollisionMargin = 0.001 */
    double sphere_half;                     /* half extent of the TG_BP_SPHERE / TG_BP_BALL asset boxes (= the asset's radius) */
    double ball_radius;                     /* TG_BP_BALL: the ball's radius in the world */
    int32_t n_hull_verts;
    int32_t every_step;                     /* 1: the check is a node of every tg_step / tg_step_random (after the step kernel, before any reset) */
    const double* hull_verts;               /* host, [n_hull_verts][3] */
} tg_broadphase;
int tg_set_broadphase(tg_ctx* ctx, const tg_broadphase* guard);        /* NULL: forget the guard */
int tg_check_broadphase(tg_ctx* ctx);                                   /* enqueue one check of the current state on the context's stream */
int tg_get_broadphase_totals(tg_ctx* ctx, int64_t* checks, int64_t* pairs, int64_t* hits);   /* env-checks run, stage-1 pairs and hits found since tg_set_broadphase (synchronises) */
/* Draws the current state of every env now (render() in the other observation modes). Asynchronous. */
int tg_render_scene(tg_ctx* ctx);
/* uint8 [num_envs][H][W][3]; terminal != 0: the image of the last step of the envs that finished (rows valid where done). */
int tg_get_obs_visual(tg_ctx* ctx, void** dev_ptr, int32_t terminal);
int tg_copy_obs_visual(tg_ctx* ctx, uint8_t* host_dst, int32_t terminal);

/* ---- function-level entry points (parity tests call the device implementations through these) --------------------- */
/* calculateInverseDynamics (base_robot_arm.py:176-178), batch of n states; physics_dtype as in tg_config. */
int tg_inverse_dynamics(const tg_robot* robot, int32_t physics_dtype, int32_t n, const double* q, const double* qd,
                        const double* qdd, double* tau);
/* joint-space inertia matrix, [n][ndof][ndof]. */
int tg_mass_matrix(const tg_robot* robot, int32_t physics_dtype, int32_t n, const double* q, double* M);
/* calculateJacobian at the TCP frame (base_robot_arm.py:300-307): J [n][6][ndof]; also TCP pose [n][3], [n][9]. */
int tg_jacobian_tcp(const tg_robot* robot, int32_t physics_dtype, int32_t n, const double* q, double* J, double* pos,
                    double* rot);
/* n_ticks x stepSimulation (robot.py:131-141) with gravity compensation and velocity (mode 1) or position (mode 2)
 * motors; q, qd updated in place ([n][ndof]). */
int tg_sim_ticks(const tg_robot* robot, int32_t physics_dtype, int32_t n, int32_t n_ticks, int32_t solver_iterations,
                 double dt, int32_t motor_mode, const double* q_des, const double* qd_des, double max_force, double* q,
                 double* qd);
/* calculateInverseKinematics at the TCP frame (base_robot_arm.py:201-209, maxNumIterations=100, residualThreshold=1e-8):
 * q0 [n][ndof] start, target_pos [n][3], target_rot [n][9] row-major -> q_out [n][ndof], iters [n] (nullable). */
int tg_inverse_kinematics(const tg_robot* robot, int32_t physics_dtype, int32_t n, const double* q0, const double* target_pos,
                          const double* target_rot, int32_t max_iters, double threshold, double* q_out, int32_t* iters);
/* getCameraImage depth + t_s_camera (tactile_sensor.py:239-294) for n transforms [n][12] -> uint8 [n][h][w]. */
int tg_render_tactile(const tg_sensor* sensor, const tg_mesh* mesh, int32_t n, const float* cam_from_obj, uint8_t* out);
/* Same for a per-image heightfield stimulus (createCollisionShape(GEOM_HEIGHTFIELD), base_surface_env.py:402-432):
 * heights [n][rows*cols] (double, heightfield_data[row][col]), zoff [n]. */
int tg_render_tactile_heightfield(const tg_sensor* sensor, int32_t rows, int32_t cols, double grid_scale, int32_t n,
                                  const double* heights, const float* zoff, const float* cam_from_obj, uint8_t* out);
/* gen_heigtfield_simplex_2d (base_surface_env.py:319-337) for n seeds: heights [n][rows*cols], zoff [n] (nullable). */
int tg_gen_heightfield(int32_t n, const int64_t* seeds, int32_t rows, int32_t cols, double interp, double range, double* heights,
                       float* zoff);

/* action_space.sample() for the whole batch (the reference's demo loops draw env.action_space.sample() per env and step,
 * examples/demo_rl_env_base.py:34; Box(min_action, max_action) float32, edge_follow_env.py:169-174): dev_actions [num_envs][act_dim]
 * (device memory) receives U[min_action, max_action) draws, counter based: element i of draw `counter` is a function of
 * (seed, counter, i) only.  Enqueued on the context's stream, so a tg_step(dev_actions, on_device = 1) that follows sees it. */
int tg_sample_actions(tg_ctx* ctx, uint64_t seed, uint64_t counter, float* dev_actions);
/* A random-action rollout step (the north_star's synthetic rollout: `env.step(env.action_space.sample())`, examples/demo_rl_env_base.py:34, for the
 * whole batch): tg_sample_actions' draw followed by tg_step on it as one sequence of launches - the draw is made by the step kernel itself where the
 * lane-mapped k_step / k_step_body_wave runs, by the sequence's first launch elsewhere; the draw counter lives in device memory and moves on by one
 * per call.  The launches go on the stream one by one (until round 6 the sequence was one captured graph, but a graph launch costs ~6.6 us before
 * its first kernel starts on this stack, a launch on the stream ~2 us).  restart != 0 (or a new seed): the next step uses draw first_draw + 1.  The
 * actions are the context's own buffer (tg_get_actions: device float32 [num_envs][act_dim]); draw k equals tg_sample_actions(seed, k). */
int tg_step_random(tg_ctx* ctx, uint64_t seed, uint64_t first_draw, int32_t restart);
int tg_get_actions(tg_ctx* ctx, void** dev_actions);

/* ---- frame stack: stable_baselines3's VecFrameStack(venv, n_stack) on the device (sb3_helpers/rl_utils.py:32, 65; ABI v15) -------------------------
 * tg_set_frame_stack(n), 2 <= n <= 8: every observation key is also kept as a stack of its last n frames along its last axis, oldest first - tactile
 * uint8 [num_envs][H][W][n], oracle float32 [num_envs][dim * n] (when tg_enable_oracle_obs was called first), extended_feature float32
 * [num_envs][feature_dim * n] (push 12, roll 3, surface_follow 6 of the 12-wide rows).  tg_reset zeroes the reset envs' stacks and puts the reset
 * observation in the newest slot.  Every tg_step / tg_step_random shifts every stack one slot toward the oldest and puts the step's observation in the
 * newest slot; an env that is done first has its stack zeroed and, with auto_reset, its terminal stack written: the old stack's newest n - 1 slots,
 * then the terminal observation (rows valid where done).  One launch per step / reset, after the observations.  n = 1 frees the stacks (no launch).
 * Refused together with tg_set_obs_targets.  TG_STACK_REWRITE_ALL=1 (read once per process) turns off the kernel's unchanged-block skip. */
#define TG_OBS_KEY_TACTILE 0
#define TG_OBS_KEY_ORACLE 1
#define TG_OBS_KEY_FEATURE 2
int tg_set_frame_stack(tg_ctx* ctx, int32_t n);
int tg_get_frame_stack(tg_ctx* ctx, int32_t* n);
int tg_get_obs_stack(tg_ctx* ctx, int32_t key, int32_t terminal, void** dev_ptr);
int tg_copy_obs_stack(tg_ctx* ctx, int32_t key, int32_t terminal, void* host_dst);                /* synchronises */
/* The stacks of `count` chosen envs only (the finished envs' terminal stacks): env_ids[k]'s row goes to host_dst + k * row_bytes. */
int tg_copy_obs_stack_rows(tg_ctx* ctx, int32_t key, int32_t terminal, const int32_t* env_ids, int32_t count, void* host_dst);

/* ---- observation layout: stable_baselines3's VecTransposeImage on the device (sb3_helpers/rl_utils.py:33, 66; ABI v16) ---------------------------
 * tg_set_obs_layout(1): the image stacks are kept channels first, what VecTransposeImage(VecFrameStack(venv, n)) hands out - tactile uint8
 * [num_envs][n][H][W], visual uint8 [num_envs][3 n][H][W] (plane 3 s + c: stack slot s, oldest first, colour c).  0 (default): channels last,
 * tactile [num_envs][H][W][n], visual [num_envs][H][W][3 n].  The vector keys are the same in both layouts.
 * The visual key (TG_OBS_KEY_VISUAL) is stacked when the scene is drawn every step (tg_set_scene with every_step, the visual observation modes) and
 * n > 1 or channels first; tg_set_scene must come first, and is refused afterwards.  With n = 1 and channels first the tactile "stack" is the
 * observation buffer itself ([num_envs][H][W] is [num_envs][1][H][W]; tg_get_obs_stack returns it), and only a visual key costs a launch.
 * tg_set_frame_stack and tg_set_obs_layout may come in either order: each (re)allocates every stack for the current (n, layout), zeroed; call them
 * before the first tg_reset.  Both updates keep tg_set_frame_stack's rules and call sites: one update per tg_reset and per step, after the step's
 * tactile and scene renders.  Channels first is refused together with tg_set_obs_targets (sharded runs). */
#define TG_OBS_KEY_VISUAL 3
int tg_set_obs_layout(tg_ctx* ctx, int32_t channels_first);
int tg_get_obs_layout(tg_ctx* ctx, int32_t* channels_first);

/* ---- image augmentation: RAD's kornia RandomAffine(degrees=0, translate=[ax, ay], scale=[1, 1], p) (sb3_helpers/params/<task>_params.py:7-9) ----
 * Context free.  in_dev: a [B][C][H][W] (channels_first = 1) or [B][H][W][C] (0) batch of uint8 or float32 images (TG_AUGMENT_*) in device
 * memory; out_dev: float32, same shape and layout, not overlapping the input, which is only read.  Sample b is warped with probability p by a
 * shift of tx ~ U(-ax W, ax W), ty ~ U(-ay H, ay H) pixels as kornia's warp_affine (bilinear, zero padding, align_corners=False) applies it:
 * out[y][x] = bilinear(in, x - tx W / (W - 1), y - ty H / (H - 1)), every tap outside the image 0, all channels alike; otherwise out = in.
 * The draws are element 3 b + k of tg_sample_actions' generator at (seed, counter); params_in_dev (nullable): float32 [B][3] (apply, tx, ty)
 * used instead of the draws; params_out_dev (nullable): receives them.  H, W >= 2, 0 <= ax, ay, p <= 1; B = 0 does nothing.  Enqueued on
 * hip_stream; nothing is allocated or synchronised.  The arithmetic, bit for bit: DESIGN.md 4.8. */
#define TG_AUGMENT_UINT8 0
#define TG_AUGMENT_FLOAT32 1
int tg_random_translate(const void* in_dev, void* out_dev, int32_t in_dtype, int32_t channels_first, int64_t B, int32_t C, int32_t H, int32_t W,
                        double ax, double ay, float p, uint64_t seed, uint64_t counter, const float* params_in_dev, float* params_out_dev,
                        void* hip_stream);
/* tg_random_translate with a row-indexed source: rows_dev (nullable; device memory, int64 [B]) names the source sample of every output sample -
 * sample b reads source sample rows_dev[b] of in_dev; draws, params_in_dev / params_out_dev and the output stay indexed by b.  With p = 0 it is
 * the plain gather-and-convert to float32.  NULL rows_dev is tg_random_translate itself.  With rows the caller guarantees that every entry names
 * a sample inside in_dev's allocation and that out_dev does not overlap it (the extent of the source is not known here). */
int tg_random_translate_rows(const void* in_dev, void* out_dev, int32_t in_dtype, int32_t channels_first, int64_t B, int32_t C, int32_t H,
                             int32_t W, double ax, double ay, float p, uint64_t seed, uint64_t counter, const float* params_in_dev,
                             float* params_out_dev, const int64_t* rows_dev, void* hip_stream);

/* ---- general affine augmentation: kornia's RandomAffine(degrees, translate, scale, shear, p) with its defaults ----------------
 * Context free; images, layouts, dtypes (TG_AUGMENT_*), overlap rule and stream as tg_random_translate: one launch, nothing allocated or
 * synchronised.  Sample b is warped with probability p by a rotation of angle ~ U(d0, d1) degrees and a scale of scale_x ~ U(s0, s1), scale_y
 * ~ U(s2, s3) (s2 = s3 = 0: scale_y = scale_x) about the image centre, a shear of shear_x ~ U(h0, h1), shear_y ~ U(h2, h3) degrees about it,
 * and a shift of tx ~ U(-ax W, ax W), ty ~ U(-ay H, ay H) pixels, resampled as kornia's warp_affine does (bilinear, zero padding,
 * align_corners=False), all channels alike; otherwise out = in.  The draws are element 8 b + k of tg_sample_actions' generator at
 * (seed, counter).  params_in_dev (nullable): float32 [B][8] (apply, tx, ty, angle, scale_x, scale_y, shear_x, shear_y) used instead of the
 * draws; params_out_dev (nullable): receives them (apply as 0 / 1).  coeffs_in_dev (nullable): float32 [B][6] (a00, a01, a02, a10, a11, a12),
 * output pixel (column j, row i) samples the input at (a00 j + a01 i + a02, a10 j + a11 i + a12), used as they are instead of the ones the
 * parameters give - only `apply` is then taken from the parameters; coeffs_out_dev (nullable): receives the coefficients used.
 * H, W >= 2, 0 <= ax, ay, p <= 1, every range finite and ordered, scales > 0; B = 0 does nothing.  The arithmetic, stage by stage: DESIGN.md 4.11. */
int tg_random_affine(const void* in_dev, void* out_dev, int32_t in_dtype, int32_t channels_first, int64_t B, int32_t C, int32_t H, int32_t W,
                     double ax, double ay, float d0, float d1, float s0, float s1, float s2, float s3, float h0, float h1, float h2, float h3,
                     float p, uint64_t seed, uint64_t counter, const float* params_in_dev, float* params_out_dev, const float* coeffs_in_dev,
                     float* coeffs_out_dev, void* hip_stream);
/* tg_random_affine with a row-indexed source, as tg_random_translate_rows: sample b reads source sample rows_dev[b] (nullable: b itself);
 * draws, parameters, coefficients and the output stay indexed by b.  The caller guarantees that every entry names a sample inside in_dev's
 * allocation and that out_dev does not overlap it. */
int tg_random_affine_rows(const void* in_dev, void* out_dev, int32_t in_dtype, int32_t channels_first, int64_t B, int32_t C, int32_t H, int32_t W,
                          double ax, double ay, float d0, float d1, float s0, float s1, float s2, float s3, float h0, float h1, float h2,
                          float h3, float p, uint64_t seed, uint64_t counter, const float* params_in_dev, float* params_out_dev,
                          const float* coeffs_in_dev, float* coeffs_out_dev, const int64_t* rows_dev, void* hip_stream);

/* ---- device rollout buffer: stable_baselines3's RolloutBuffer / DictRolloutBuffer over step-major [T][N][...] device arrays ----
 * Context free; every call is ONE launch enqueued on hip_stream, nothing is allocated or synchronised.  The pointer / size tables are host arrays
 * of n_arrays <= TG_ROLLOUT_MAX_ARRAYS entries, read before the call returns; the pointers in them are device memory.
 *
 * tg_rollout_add: array i copies bytes[i] bytes from src_dev[i] to dst_dev[i] (TG_ROLLOUT_COPY), or reads bytes[i] uint8 flags and writes as
 * many float32 0.0 / 1.0 (TG_ROLLOUT_FLAG_U8; dst 4-byte aligned): the observation keys and per-env rows of one step into their slot.  16-byte
 * accesses where both pointers and the byte count allow, 4-byte or single bytes otherwise.  No destination may overlap its source.
 *
 * tg_rollout_gae: SB3's GAE(lambda) over float32 [T][N] rewards / values / episode_starts, float32 [N] last_values and [N] dones (uint8 or
 * float32, non-zero = done), writing float32 [T][N] advantages and returns.  Per env, t = T-1 ... 0, float32, one rounding per operation, no fused
 * multiply-add, g = (float)gamma, gl = (float)(gamma * gae_lambda):
 *     nnt = 1 - (t == T-1 ? dones : episode_starts[t+1]);   nv = t == T-1 ? last_values : values[t+1]
 *     delta = (rewards[t] + (g * nv) * nnt) - values[t];    last = delta + (gl * nnt) * last   (last = 0 before t = T-1)
 *     advantages[t] = last;                                 returns[t] = last + values[t]
 *
 * tg_rollout_gather: for every array i and b < B, row b of dst_dev[i] = row rows_dev[b] of src_dev[i], rows of row_bytes[i] bytes (one minibatch
 * of every array that is not an image key).  rows_dev: device memory, int64 [B], every entry a row inside each source (not checked). */
#define TG_ROLLOUT_MAX_ARRAYS 16
#define TG_ROLLOUT_COPY 0
#define TG_ROLLOUT_FLAG_U8 1
#define TG_ROLLOUT_DONES_UINT8 0
#define TG_ROLLOUT_DONES_FLOAT32 1
int tg_rollout_add(int32_t n_arrays, const void* const* src_dev, void* const* dst_dev, const int64_t* bytes, const int32_t* kinds, void* hip_stream);
int tg_rollout_gae(const float* rewards_dev, const float* values_dev, const float* episode_starts_dev, const float* last_values_dev,
                   const void* dones_dev, int32_t dones_dtype, float* advantages_dev, float* returns_dev, int64_t T, int64_t N, double gamma,
                   double gae_lambda, void* hip_stream);
int tg_rollout_gather(int32_t n_arrays, const void* const* src_dev, void* const* dst_dev, const int64_t* row_bytes, const int64_t* rows_dev,
                      int64_t B, void* hip_stream);

/* ---- device replay buffer: stable_baselines3's ReplayBuffer / DictReplayBuffer over step-major [T][N][...] device rings ----
 * Context free; every call is ONE launch enqueued on hip_stream, nothing is allocated or synchronised.  The tables are host arrays of
 * n_arrays <= TG_ROLLOUT_MAX_ARRAYS entries, read before the call returns; the pointers in them are device memory.
 *
 * tg_replay_add: array i has n_rows rows of row_bytes[i] bytes, back to back in src_dev[i], alt_dev[i] and dst_dev[i].  Destination row n is row n
 * of alt_dev[i] when alt_dev[i] != NULL && select_dev[n] (uint8 [n_rows], non-zero = take alt), else row n of src_dev[i]; only the chosen source
 * of a row is read.  TG_ROLLOUT_COPY copies the bytes; TG_ROLLOUT_FLAG_U8 (row_bytes[i] = 1) reads one uint8 per row and writes one float32
 * 0.0 / 1.0 (dst 4-byte aligned).  select_dev may be NULL when every alt_dev[i] is.  16-byte accesses where the row byte count and the three
 * addresses allow, 4-byte or single bytes otherwise.  No destination may overlap a source of its array.  One transition batch of a replay
 * buffer: next_observations[pos] (alt = the terminal observations, select = the done flags), actions, rewards, dones, timeouts, and - an
 * array like the others with a NULL alt - observations[pos + 1].
 *
 * tg_replay_draw: the counter-based draw of a minibatch, on tg_sample_actions' generator.  For b < B:
 *     h = mix64(mix64(seed + G (counter + 1)) + G (b + 1));     G = 0x9E3779B97F4A7C15
 *     t = (first_slot + (((h >> 32) * n_slots) >> 32)) % T;       n = ((h & 0xffffffff) * N) >> 32;      row = t N + n
 *     rows_dev[b] = row;   rows_dev[B + b] = row + next_offset                        (int64 [2 B]; all of it 64-bit integer arithmetic)
 *     actions_out[b][0 .. A) = actions_dev[row][0 .. A);   rewards_out[b] = rewards_dev[row];
 *     dones_out[b] = dones_dev[row] * (1 - timeouts_dev[row])                        (float32, one rounding per operation)
 * 1 <= n_slots <= T, n_slots and N below 2^31, T N <= 2^40, 0 <= first_slot < T.  actions_dev, rewards_dev, dones_dev and timeouts_dev may be
 * NULL together: then only the rows are written (and the three outputs are not touched). */
int tg_replay_add(int32_t n_arrays, const void* const* src_dev, const void* const* alt_dev, void* const* dst_dev, const int64_t* row_bytes,
                  const int32_t* kinds, int64_t n_rows, const void* select_dev, void* hip_stream);
int tg_replay_draw(int64_t B, int64_t n_slots, int64_t first_slot, int64_t T, int64_t N, uint64_t seed, uint64_t counter,
                   const float* actions_dev, int32_t A, const float* rewards_dev, const float* dones_dev, const float* timeouts_dev,
                   int64_t next_offset, int64_t* rows_dev, float* actions_out, float* rewards_out, float* dones_out, void* hip_stream);

/* ---- device VecNormalize: stable_baselines3's VecNormalize / RunningMeanStd over float32 device arrays, statistics in float64 ----
 * Context free; enqueued on hip_stream, nothing is allocated or synchronised.  The tables are host arrays of n_arrays <= TG_VECNORM_MAX_ARRAYS
 * entries, read before the call returns; the pointers in them are device memory.  Array i is float32 [rows][widths[i]], widths[i] >= 1 and the
 * widths add up to at most TG_VECNORM_MAX_WIDTH; stats_dev[i] is its block of 2 widths[i] + 1 doubles: mean [d] | var [d] | count.  ret_stats_dev
 * is the block of the discounted return: mean, var, count.  Every operation is float64 with one rounding; the order of the sums is DESIGN.md
 * 4.12's (tests/vecnorm_ref.py restates it bit for bit).
 *
 * tg_vecnorm_update (TWO launches): RunningMeanStd.update of every array with its N rows, 1 <= N <= TG_VECNORM_MAX_ROWS.  With returns_dev
 * (float64 [N]), rewards_dev (float32 [N]) and ret_stats_dev - NULL together or not at all - also returns = returns gamma + rewards, written back,
 * and the update of ret_stats with the new returns as an [N][1] batch.  scratch_dev: 2 ((N + 255) / 256) (sum of widths + 1) doubles of the
 * caller's, overwritten.
 *
 * tg_vecnorm_apply (ONE launch): out_dev[i][r][j] = (float) clip(((double) x_dev[i][r][j] - mean[j]) / sqrt(var[j] + epsilon), -clip_obs, clip_obs)
 * for r < R (any row count up to TG_VECNORM_MAX_APPLY_ROWS; out_dev[i] may be x_dev[i]).  With rewards_dev: rewards_out[e] = (float)
 * clip((double) rewards_dev[e] / sqrt(ret var + epsilon), -clip_reward, clip_reward) for e < n_rewards (rewards_out may be rewards_dev).  With
 * returns_dev: returns_dev[e] = 0 for e < n_reset where dones_dev[e] (uint8), everywhere when dones_dev is NULL. */
#define TG_VECNORM_MAX_ARRAYS 4
#define TG_VECNORM_MAX_WIDTH 512
#define TG_VECNORM_MAX_ROWS 65535
#define TG_VECNORM_MAX_APPLY_ROWS 2147483647
int tg_vecnorm_update(int32_t n_arrays, const float* const* x_dev, const int32_t* widths, double* const* stats_dev, int64_t N, double* returns_dev,
                      const float* rewards_dev, double gamma, double* ret_stats_dev, double* scratch_dev, void* hip_stream);
int tg_vecnorm_apply(int32_t n_arrays, const float* const* x_dev, float* const* out_dev, const int32_t* widths, const double* const* stats_dev,
                     int64_t R, double clip_obs, double epsilon, const float* rewards_dev, float* rewards_out, int64_t n_rewards,
                     const double* ret_stats_dev, double clip_reward, double* returns_dev, const uint8_t* dones_dev, int64_t n_reset,
                     void* hip_stream);

/* ---- device action heads: what stable_baselines3 does between the policy's output and venv.step(), use_sde=False --------------
 * Context free; ONE launch on hip_stream, nothing is allocated or synchronised.  mean_dev: float32 [N][A]; log_std_dev: float32 [A] with
 * log_std_stride 0 (PPO's state-independent parameter) or [N][A] with log_std_stride A (SAC's network output), clamped to
 * [log_std_min, log_std_max] first (-inf / +inf: no clamp); lo, hi: the action space's bounds, float32 host arrays of A entries read before the
 * call returns.  Float32 arithmetic with one rounding per operation; exp, tanh, log and the draw are evaluated in double on the float32 argument
 * and rounded to float32 once.  With ls the clamped log_std, sigma = (float) exp(ls), eps the draw and x = mean + sigma eps:
 *   TG_HEAD_GAUSSIAN  (DiagGaussianDistribution, PPO)   actions = x;  env = min(max(x, lo), hi) (np.clip; a NaN passes);
 *                     log_prob[i] = sum_j (-(x - mean)^2 / (2 sigma^2) - ls - log sqrt(2 pi)), float32, j ascending
 *   TG_HEAD_SQUASHED  (SquashedDiagGaussianDistribution, SAC)   a = (float) tanh(x);  actions = a;  env = lo + 0.5 (a + 1) (hi - lo)
 *                     (unscale_action), clipped to [lo, hi] (the float32 formula can leave it by one rounding at a = +-1);
 *                     log_prob[i] = the Gaussian sum - sum_j (float) log(1 - a a + 1e-6f)
 *   TG_HEAD_UNIFORM   (SAC before learning_starts)   env = lo + (hi - lo) u, u = 24 bits 2^-24 of element e = i A + j of tg_sample_actions'
 *                     generator at (seed, counter), at most hi;  actions = 2 ((env - lo) / (hi - lo)) - 1 (scale_action).  mean_dev and log_std_dev are
 *                     not read (they may be NULL); gaussian_out and log_prob_out are not written.
 * The draw: k1, k2 = the 24 bits of elements 2 e and 2 e + 1;  eps = (float) (sqrt(-2 log((k1 + 1) 2^-24)) cos(2 pi k2 2^-24)), in double;
 * |eps| <= 5.77.  deterministic != 0: eps = 0.  noise_in_dev (nullable, float32 [N][A]) is used in place of the draws (of u in the uniform
 * mode).  Every output is nullable: actions_out, env_actions_out, gaussian_out (x), noise_out [N][A], log_prob_out [N].  N = 0 does nothing.
 * Errors, each without a launch: NULL mean_dev or log_std_dev in a Gaussian mode, A outside [1, TG_HEAD_MAX_ACT], a stride other than 0 or A,
 * lo[j] > hi[j], lo[j] == hi[j] in the squashed or uniform mode, log_std_min > log_std_max, an unknown mode. */
#define TG_HEAD_GAUSSIAN 0
#define TG_HEAD_SQUASHED 1
#define TG_HEAD_UNIFORM 2
#define TG_HEAD_MAX_ACT 16
#define TG_HEAD_MAX_ROWS 2147483647
int tg_action_head(const float* mean_dev, const float* log_std_dev, int32_t log_std_stride, int64_t N, int32_t A, const float* lo, const float* hi,
                   float log_std_min, float log_std_max, int32_t mode, int32_t deterministic, uint64_t seed, uint64_t counter,
                   const float* noise_in_dev, float* actions_out, float* env_actions_out, float* gaussian_out, float* log_prob_out,
                   float* noise_out, void* hip_stream);

/* ---- device conv stem: NatureCNN's first layer on this project's observations -------------------------------------------------
 * stable_baselines3's preprocess_obs (obs.float() / 255), Conv2d(Cn, 32, kernel_size=8, stride=4) and ReLU as ONE launch, and the layer's
 * backward pass for the weight and the bias (the input is data: there is no input gradient).  Context free; the launches go to hip_stream,
 * nothing is allocated or synchronised.  x_dev: uint8 (x_is_float 0) or float32 (x_is_float 1), [B][Cn][H][W] (channels_first 1) or
 * [B][H][W][Cn] (channels_first 0); weight_dev: float32 [32][Cn][8][8] (torch's Conv2d layout); bias_dev: float32 [32]; y_dev: float32
 * [B][32][OH][OW], OH = (H - 8) / 4 + 1, OW = (W - 8) / 4 + 1 (floor: trailing input rows and columns are not read).  Per output element,
 * with k = (c 8 + ky) 8 + kx and K = 64 Cn:
 *     acc = 0;  for k = 0 .. K-1 ascending: acc = fmaf((float) x_k, w[co][k], acc);  y = fmaxf(fmaf(acc, scale, bias[co]), 0)
 * in float32, bit for bit, whatever B is and wherever the image sits in the batch (scale: 1 / 255 for uint8 images).
 *
 * The backward call (at most TWO launches): with g = dy (y > 0),  dbias[co] = sum of g,  dweight[co][k] = scale * sum over (b, oy, ox) of
 * g (float) x_k.  The sums are split over workgroups into partials in workspace_dev (the caller's, at least the size that
 * tg_conv_stem_bwd_workspace (B, Cn, H, W) returns, in bytes; overwritten) and reduced in a fixed order without atomics: the same inputs give
 * the same bits on every run.  dweight_dev: float32 [32][Cn][8][8]; dbias_dev: float32 [32]; both overwritten.
 * B = 0 does nothing.  Errors, each without a launch: a NULL pointer, Cn outside [1, TG_STEM_MAX_CIN], H < 8 or W < 8, B < 0, more than
 * 2^24 - 1 workgroups' worth of output (128 output positions each), a workspace that is too small (the size query returns the negative code). */
#define TG_STEM_KERNEL 8
#define TG_STEM_STRIDE 4
#define TG_STEM_OUT 32
#define TG_STEM_MAX_CIN 12
int tg_conv_stem(const void* x_dev, int32_t x_is_float, int32_t channels_first, int64_t B, int32_t Cn, int32_t H, int32_t W,
                 const float* weight_dev, const float* bias_dev, float scale, float* y_dev, void* hip_stream);
int64_t tg_conv_stem_bwd_workspace(int64_t B, int32_t Cn, int32_t H, int32_t W);
int tg_conv_stem_bwd(const void* x_dev, int32_t x_is_float, int32_t channels_first, int64_t B, int32_t Cn, int32_t H, int32_t W,
                     const float* y_dev, const float* dy_dev, float scale, float* dweight_dev, float* dbias_dev, void* workspace_dev,
                     int64_t workspace_bytes, void* hip_stream);

/* ---- device NatureCNN tail: conv2, conv3 and the linear layer as one kernel family ----------------------------------------------
 * A valid (unpadded) strided convolution with bias and ReLU.  Context free; the launches go to hip_stream, nothing is allocated or
 * synchronised.  x_dev: float32 [B][Cin][H][W], contiguous; weight_dev: float32 [Cout][Cin][KH][KW] (torch's layout); bias_dev: float32 [Cout];
 * y_dev: float32 [B][Cout][OH][OW], OH = (H - KH) / stride + 1, OW = (W - KW) / stride + 1 (floor).  NatureCNN's Conv2d(32, 64, 4, 2) and
 * Conv2d(64, 64, 3, 1) are instances; Flatten + Linear(64 h w, F) is the instance Cin = 64, H = KH = h, W = KW = w, Cout = F, stride 1
 * (OH = OW = 1, K = 64 h w): nn.Linear's [F][64 h w] weight is that kernel, flattened.  Per output element, with k = (c KH + ky) KW + kx and
 * K = Cin KH KW:
 *     acc = 0;  for k = 0 .. K-1 ascending: acc = fmaf(x_k, w[co][k], acc);  z = acc + b[co];  y = z > 0 ? z : (z != z ? z : 0)
 * in float32, bit for bit: ONE chain for every shape (K is not cut into segments), so an element's arithmetic order is a function of the
 * layer's shape alone - never of B, of the row's index or of where its tile falls.  ONE launch.
 *
 * The backward call (at most THREE launches: partials, reduction, dx): with g = dy where y > 0 and 0 elsewhere (y_dev: the forward's output),
 *     dbias[co] = sum_m g[m][co],   dweight[co][k] = sum_m g[m][co] x[m][k],   m = (b OH + oy) OW + ox
 * split over workgroups into partials in workspace_dev (the caller's, at least tg_conv_relu_bwd_workspace(...) bytes; overwritten) and reduced
 * in a fixed order without atomics: the same inputs give the same bits on every run.  The number of partials grows with M = B OH OW:
 * P = max(1, min(ceil(M / 256), 64, 2^25 / (Cout K))), the workspace is 4 P (Cout K + 4 Cout) bytes.  And
 *     dx[b][c][iy][ix] = one chain over j = (co KH + ky) KW + kx ascending of g[b][co][oy][ox] w[co][c][ky][kx],
 *     oy = (iy - ky) / stride, ox = (ix - kx) / stride;  a term whose division is inexact or whose (oy, ox) is outside the output is fed as
 *     0 w or skipped (the same bits for finite w), so input rows and columns that no output reads get 0.
 * dx_dev may be NULL: then no dx kernel is launched (frozen upstream layers).  dweight_dev [Cout][Cin][KH][KW], dbias_dev [Cout] and dx_dev
 * [B][Cin][H][W] are overwritten.  B = 0 does nothing.  Errors, each without a launch: a NULL pointer (but dx_dev), Cin outside
 * [1, TG_CONV_MAX_CIN], Cout no multiple of TG_CONV_COUT_STEP or above TG_CONV_MAX_COUT, KH or KW outside [1, TG_CONV_MAX_KERNEL] or larger
 * than H or W, stride outside [1, TG_CONV_MAX_STRIDE], an odd K (the MFMA takes two k per instruction), B < 0, B H W above TG_CONV_MAX_POSITIONS
 * (one launch), a workspace that is too small (the size query returns the negative code). */
#define TG_CONV_MAX_CIN 64
#define TG_CONV_COUT_STEP 32
#define TG_CONV_MAX_COUT 512
#define TG_CONV_MAX_KERNEL 16
#define TG_CONV_MAX_STRIDE 4
#define TG_CONV_MAX_POSITIONS 536870880
int tg_conv_relu(const float* x_dev, int64_t B, int32_t Cin, int32_t H, int32_t W, const float* weight_dev, const float* bias_dev, int32_t Cout,
                 int32_t KH, int32_t KW, int32_t stride, float* y_dev, void* hip_stream);
int64_t tg_conv_relu_bwd_workspace(int64_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t KH, int32_t KW, int32_t stride);
int tg_conv_relu_bwd(const float* x_dev, int64_t B, int32_t Cin, int32_t H, int32_t W, const float* weight_dev, const float* y_dev,
                     const float* dy_dev, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, float* dweight_dev, float* dbias_dev,
                     float* dx_dev, void* workspace_dev, int64_t workspace_bytes, void* hip_stream);

/* ---- device loss heads: what stable_baselines3 does between the network's output and the scalar loss ---------------------------
 * Context free; the launches go to hip_stream, nothing is allocated or synchronised.  Float32 arithmetic with one rounding per operation; exp,
 * tanh and log are evaluated in double on the float32 argument and rounded once.  Every sum over rows is taken in double and rounded to float32
 * once: rows in chunks of 256 consecutive rows, a fixed lane tree inside a chunk, the chunk sums added in ascending order, no atomics - the same
 * inputs give the same bits on every run and on both paths.
 *
 * tg_ppo_loss: PPO.train from evaluate_actions to `loss`.  mean_dev, actions_dev: float32 [B][A]; log_std_dev: [A] (log_std_stride 0) or [B][A]
 * (log_std_stride A), not clamped; values_dev, old_log_prob_dev, advantages_dev, returns_dev: [B]; old_values_dev: [B], needed when
 * clip_range_vf >= 0 (negative: no value clip).  Per row, with d = actions - mean and sigma = (float) exp(log_std):
 *     log_prob = sum_j (-d^2 / (2 sigma^2) - log_std - log sqrt(2 pi))       tg_action_head's TG_HEAD_GAUSSIAN chain: its bits on its own sample
 *     entropy  = sum_j (1.4189385332046727f + log_std)
 *     adv      = (advantages - adv_mean) / (adv_std + 1e-8f) when normalize_advantage != 0 and B > 1 (the unbiased std), else advantages
 *     ratio    = (float) exp(log_prob - old_log_prob);   surrogate = min(adv ratio, adv clamp(ratio, 1 - clip_range, 1 + clip_range))
 *     values_pred = values, or old_values + clamp(values - old_values, -clip_range_vf, clip_range_vf)
 * stats_out, float32 [8]: loss = policy_loss + ent_coef entropy_loss + vf_coef value_loss, policy_loss = -mean(surrogate), value_loss =
 * mean((returns - values_pred)^2), entropy_loss = -mean(entropy), approx_kl = mean((ratio - 1) - (log_prob - old_log_prob)), clip_fraction =
 * mean(|ratio - 1| > clip_range), adv_mean, adv_std (0 and 1 when the advantages are not normalised).  Nullable: log_prob_out [B] and the
 * gradients of loss by torch autograd's rules, dmean_out [B][A], dlog_std_out ([A], summed over rows in the chunk order, or [B][A]) and
 * dvalues_out [B]; advantages, returns, old values and old log-probs are data.  path: TG_LOSS_PATH_ONE, one workgroup and one launch
 * (B <= TG_LOSS_ONE_MAX_ROWS); TG_LOSS_PATH_GRID, three launches with the chunk sums in workspace_dev (the caller's, at least the bytes that
 * tg_ppo_loss_workspace (B, A) returns; overwritten); TG_LOSS_PATH_AUTO, the first where it applies.
 * Errors, each without a launch: a NULL input or stats_out, A outside [1, TG_HEAD_MAX_ACT], a stride other than 0 or A, B < 1, clip_range < 0
 * or a NaN, clip_range_vf >= 0 without old_values_dev, an unknown path, TG_LOSS_PATH_ONE with too many rows, a workspace that is missing or
 * too small on the grid path (the size query returns the negative code).
 *
 * tg_squashed_rsample: SAC's actor.action_log_prob, TG_HEAD_SQUASHED's arithmetic at (seed, counter) (noise_in_dev as there): actions_out
 * [B][A] and log_prob_out [B], and for the backward pass (nullable) eps_out and sigma_out [B][A].  tg_squashed_rsample_bwd: from
 * g_actions_dev [B][A] and g_log_prob_dev [B] (each nullable: zero), the saved actions, eps, sigma and the forward's log_std_dev, with
 * w = (1 - a^2) + 1e-6f and s = g_a (1 - a^2) + g_lp 2 a (1 - a^2) / w:  dmean_out = s,  dlog_std_out = (s sigma eps - g_lp) m, both
 * [B][A] and nullable, m = 1 where log_std lies in [log_std_min, log_std_max] (inclusive, torch.clamp's rule) and 0 elsewhere.  One launch each.
 * Non-finite values follow torch's autograd: with g_log_prob_dev, s is NaN where g_lp (sigma eps) / sigma^2 is not finite,
 * and eps_out is NaN where mean is not finite (the noise, bit for bit, everywhere else). */
#define TG_LOSS_PATH_AUTO 0
#define TG_LOSS_PATH_ONE 1
#define TG_LOSS_PATH_GRID 2
#define TG_LOSS_ONE_MAX_ROWS 4096
int64_t tg_ppo_loss_workspace(int64_t B, int32_t A);
int tg_ppo_loss(const float* mean_dev, const float* log_std_dev, int32_t log_std_stride, const float* values_dev, const float* actions_dev,
                const float* old_log_prob_dev, const float* advantages_dev, const float* returns_dev, const float* old_values_dev, int64_t B,
                int32_t A, float clip_range, float clip_range_vf, float ent_coef, float vf_coef, int32_t normalize_advantage, int32_t path,
                float* stats_out, float* log_prob_out, float* dmean_out, float* dlog_std_out, float* dvalues_out, void* workspace_dev,
                int64_t workspace_bytes, void* hip_stream);
int tg_squashed_rsample(const float* mean_dev, const float* log_std_dev, int32_t log_std_stride, int64_t B, int32_t A, float log_std_min,
                        float log_std_max, uint64_t seed, uint64_t counter, const float* noise_in_dev, float* actions_out, float* log_prob_out,
                        float* eps_out, float* sigma_out, void* hip_stream);
int tg_squashed_rsample_bwd(const float* g_actions_dev, const float* g_log_prob_dev, const float* actions_dev, const float* eps_dev,
                            const float* sigma_dev, const float* log_std_dev, int32_t log_std_stride, int64_t B, int32_t A, float log_std_min,
                            float log_std_max, float* dmean_out, float* dlog_std_out, void* hip_stream);

/* ---- SAC's device losses: SAC.train between the networks' outputs and its scalar losses ----------------------------------------
 * Context free; one launch each on hip_stream, nothing is allocated or synchronised.  The arithmetic rules of the loss heads above: float32 with
 * one rounding per operation in the order written, exp in double on the float32 argument and rounded once, every mean over rows accumulated in
 * double in the chunk order (256 consecutive rows, the lane tree, the wave sums in wave order, the chunks ascending) and rounded once, no
 * atomics.  One workgroup walks the chunks for every 1 <= B <= TG_SAC_MAX_ROWS.  The critics' outputs are n_critics separate float32 [B]
 * device arrays (1 <= n_critics <= TG_SAC_MAX_CRITICS), named by HOST arrays of n_critics device pointers, read before the call returns.
 * alpha, the entropy coefficient: (float) exp((double) *log_ent_coef_dev) where log_ent_coef_dev (a float32 device scalar) is given, else the
 * argument ent_coef.  alpha is data in both losses (SB3 detaches it).
 *
 * tg_sac_critic_loss.  Per row: m = fminf chain over q_next_i, i ascending;  y = m - alpha next_log_prob;  target = rewards +
 * ((1 - dones) gamma) y;  e_i = q_cur_i - target.  mse_i = (float) (sum_b (double) (e_i e_i) / B);  critic_loss = 0.5f (((0 + mse_0) +
 * mse_1) + ...).  stats_out, float32 [8]: critic_loss, ent_coef (alpha), target_q_mean, min_next_q_mean, mse_0 .. mse_3 (0 beyond n_critics).
 * Nullable: target_out [B];  dq_cur_out, a host array of n_critics device pointers, each nullable: dq_cur_i [B] = e_i / (float) B, the
 * gradient of critic_loss.  The target, rewards, dones and the target networks' outputs are data.
 *
 * tg_sac_actor_loss.  Per row: m = min_i q_pi_i, k the lowest index that attains it;  a = alpha log_prob - m;  c = log_prob + target_entropy.
 * actor_loss = (float) (sum a / B);  with want_ent_coef_loss != 0 (log_ent_coef_dev is then required) ent_coef_loss = -(float) (sum (double)
 * (log_ent_coef c) / B) and dlog_ent_coef = -(float) (sum c / B).  stats_out, float32 [8]: actor_loss, ent_coef_loss, ent_coef (alpha),
 * log_prob_mean, min_q_pi_mean, dlog_ent_coef, 0, 0 (ent_coef_loss and dlog_ent_coef 0 when not asked).  Nullable, for an upstream gradient
 * of 1: dlog_prob_out [B] = alpha / (float) B;  dq_pi_out, a host array of n_critics device pointers, each nullable: dq_pi_i [B] =
 * -1 / (float) B where i == k, else 0 (torch.min(dim)'s rule).
 * Errors, each without a launch: n_critics or B out of range, a NULL input, pointer array, critic output or stats_out, the entropy-coefficient
 * loss asked without log_ent_coef_dev. */
#define TG_SAC_MAX_CRITICS 4
#define TG_SAC_MAX_ROWS 65536
int tg_sac_critic_loss(const float* const* q_cur_dev, const float* const* q_next_dev, int32_t n_critics, const float* next_log_prob_dev,
                       const float* rewards_dev, const float* dones_dev, int64_t B, float gamma, const float* log_ent_coef_dev, float ent_coef,
                       float* stats_out, float* target_out, float* const* dq_cur_out, void* hip_stream);
int tg_sac_actor_loss(const float* log_prob_dev, const float* const* q_pi_dev, int32_t n_critics, int64_t B, const float* log_ent_coef_dev,
                      float ent_coef, float target_entropy, int32_t want_ent_coef_loss, float* stats_out, float* dlog_prob_out,
                      float* const* dq_pi_out, void* hip_stream);

/* ---- device Adam: torch.nn.utils.clip_grad_norm_ and torch.optim.Adam's step over a list of tensors ----------------------------
 * Context free; the launches go to hip_stream, nothing is allocated or synchronised.  The tensors are n_tensors (>= 1) separate contiguous float32
 * device arrays of counts[i] >= 1 elements, named by HOST arrays of device pointers; counts, step_size and bias_corr2_sqrt are host arrays too,
 * all read before the call returns.  The tensors are cut into chunks of TG_OPTIM_CHUNK elements, a tensor's last chunk short, a chunk never
 * across two tensors; the chunks are numbered in the order of the call and one workgroup takes one chunk.  The kernels take their tensor
 * table by value, TG_OPTIM_MAX_TENSORS tensors a launch: more tensors are more launches, nothing else.
 *
 * tg_optim_sumsq: partials_dev[c] = the sum over chunk c of (double) g (double) g, for every chunk of the call (the caller's memory, at least
 * the bytes that tg_optim_workspace returns for the call's chunk count).  Lane t of 256 adds elements 4 (256 k + t) + j of the chunk, k = 0 ..
 * 3 outer, j = 0 .. 3 inner; the lanes by the tree v[i] += v[i + off], off = 32 .. 1 inside each wave, then the four wave sums in wave order: an
 * order that depends on the counts alone, not on the addresses.
 *
 * tg_optim_adam: with clip != 0, sum = ((0 + partials[0]) + partials[1]) + ... over n_partials (the chunk count of the tg_optim_sumsq call,
 * which may have covered more tensors than this call), total = (float) sqrt(sum), coef = max_norm / (total + 1e-6f), 1 where that exceeds 1 (a
 * NaN stays); *total_norm_out = total.  Every workgroup forms these itself, in that order.  Then per element, in float32 with one rounding
 * per operation, w1 = (float) (1 - beta1), w2 = (float) (1 - beta2), b2 = (float) beta2:
 *     g' = g coef (clip != 0);  g'' = g' + weight_decay p (weight_decay != 0);  m = m + w1 (g'' - m);  v = v b2 + w2 (g'' g'');
 *     den = sqrt(v) / bias_corr2_sqrt[i] + eps;  p = p + step_size[i] (m / den)
 * with the caller's step_size[i] = (float) (-lr / (1 - beta1^step)) and bias_corr2_sqrt[i] = (float) sqrt(1 - beta2^step) of tensor i.  g is
 * read, never written.  Errors, each without a launch: n_tensors < 1, a NULL array or tensor, a count < 1, more than 2^31 - 1 chunks; for
 * tg_optim_sumsq a NULL or too small partials_dev; for tg_optim_adam with clip != 0 a max_norm that is negative or a NaN, a NULL partials_dev
 * or total_norm_out, n_partials < 1.  tg_optim_workspace returns the negative code for a chunk count < 1. */
#define TG_OPTIM_CHUNK 4096
#define TG_OPTIM_MAX_TENSORS 64
int64_t tg_optim_workspace(int64_t n_chunks);
int tg_optim_sumsq(int32_t n_tensors, const float* const* grads_dev, const int64_t* counts, double* partials_dev, int64_t workspace_bytes,
                   void* hip_stream);
int tg_optim_adam(int32_t n_tensors, float* const* params_dev, const float* const* grads_dev, float* const* exp_avg_dev,
                  float* const* exp_avg_sq_dev, const int64_t* counts, const float* step_size, const float* bias_corr2_sqrt, double beta1,
                  double beta2, float eps, float weight_decay, int32_t clip, float max_norm, const double* partials_dev, int64_t n_partials,
                  float* total_norm_out, void* hip_stream);

/* ---- device MLP towers: stable_baselines3's policy, value and critic heads -----------------------------------------------------
 * Context free; the launches go to hip_stream, nothing is allocated or synchronised.  A tower is a chain of n_layers layers (1 ..
 * TG_MLP_MAX_LAYERS):  z_l = h_{l-1} W_l^T + b_l,  h_l = act_l(z_l),  W_l torch's float32 [out][in], every out in 1 .. TG_MLP_MAX_WIDTH.  A call
 * runs T towers (1 .. TG_MLP_MAX_TOWERS) on ONE input of B rows given as two column blocks x0_dev [B][Ka] and x1_dev [B][Kb] (Kb = 0: one block,
 * x1_dev is not read), K0 = Ka + Kb in 1 .. TG_MLP_MAX_IN.  A tower's LAST layer may have a second row block (weight2, bias2, out2 rows, out +
 * out2 <= TG_MLP_MAX_WIDTH) whose outputs and gradients go to buffers of their own (h2, dweight2, dbias2).  Per output element, in float32:
 *     acc = 0;  for k = 0 .. in-1 ascending: acc = fmaf(h_{l-1}[row][k], W_l[co][k], acc);  z = acc + b_l[co]
 *     TG_MLP_ACT_NONE: h = z;  TG_MLP_ACT_RELU: h = fmaxf(z, 0);  TG_MLP_ACT_TANH: h = (float) tanh((double) z)
 * bit for bit: an output depends on its own row only, whatever B is, wherever the row sits and whatever other towers the call runs.
 * tg_mlp_forward (ONE launch) writes every layer's h [B][out] when save_all != 0 (the backward pass reads them), else only each tower's last.
 *
 * tg_mlp_backward (at most TWO launches): dh_L = dy (dy2 for the second block; NULL: zeros); for l = L .. 1:  g_l = dh_l act'(h_l)  (Tanh:
 * t = h h, u = 1 - t, g = dh u, one rounding each; ReLU: h > 0; none: 1);  dbias_l[co] = sum over rows of g_l;  dweight_l[co][k] = sum over
 * rows of g_l[row][co] h_{l-1}[row][k];  dh_{l-1}[row][k] = the fmaf chain over co ascending of g_l[row][co] W_l[co][k];  dx = the towers'
 * dh_0 added in tower order, split into dx0_dev [B][Ka] and dx1_dev [B][Kb], each nullable (both NULL: not computed).  Every dweight / dbias
 * pointer is nullable (not written).  The sums over rows run over tiles of 32 rows in ascending order without atomics, split over at most 64
 * workgroups per tower whose partials lie in workspace_dev (the caller's, at least tg_mlp_backward_workspace's bytes, which may be 0 - then
 * workspace_dev may be NULL; overwritten) and are added in ascending order: the same inputs give the same bits on every call.
 * B = 0 does nothing.  Errors, each without a launch and without a write: a NULL required pointer, T, n_layers, a width or K0 out of range,
 * in_l != out_{l-1} (in_1 != K0), a second row block on a layer that is not the last, an unknown activation, B < 0 or above TG_MLP_MAX_ROWS,
 * a workspace that is too small (the size query returns the negative code). */
#define TG_MLP_MAX_TOWERS 4
#define TG_MLP_MAX_LAYERS 4
#define TG_MLP_MAX_WIDTH 256
#define TG_MLP_MAX_IN 1024
#define TG_MLP_MAX_ROWS 2147483616
#define TG_MLP_ACT_NONE 0
#define TG_MLP_ACT_TANH 1
#define TG_MLP_ACT_RELU 2
typedef struct tg_mlp_layer {
    const float* weight;                    /* [out][in] */
    const float* bias;                      /* [out] */
    const float* weight2;                   /* the last layer's second row block [out2][in]; NULL with out2 = 0 */
    const float* bias2;                     /* [out2] */
    float* h;                               /* [B][out]: written by the forward call (the last layer's always), read by the backward call */
    float* h2;                              /* [B][out2] */
    float* dweight;                         /* the backward call's outputs, each nullable */
    float* dbias;
    float* dweight2;
    float* dbias2;
    int32_t in, out, out2, act;             /* act: TG_MLP_ACT_* */
} tg_mlp_layer;
typedef struct tg_mlp_tower {
    int32_t n_layers, reserved;
    const float* dy;                        /* backward: the gradient of the last layer's h [B][out], of h2 [B][out2]; NULL: zeros */
    const float* dy2;
    tg_mlp_layer layer[TG_MLP_MAX_LAYERS];
} tg_mlp_tower;
int tg_mlp_forward(const float* x0_dev, int32_t Ka, const float* x1_dev, int32_t Kb, int64_t B, const tg_mlp_tower* towers, int32_t T,
                   int32_t save_all, void* hip_stream);
int64_t tg_mlp_backward_workspace(int64_t B, int32_t Ka, int32_t Kb, const tg_mlp_tower* towers, int32_t T);
int tg_mlp_backward(const float* x0_dev, int32_t Ka, const float* x1_dev, int32_t Kb, int64_t B, const tg_mlp_tower* towers, int32_t T,
                    float* dx0_dev, float* dx1_dev, void* workspace_dev, int64_t workspace_bytes, void* hip_stream);
#ifdef __cplusplus
}
#endif
#endif
