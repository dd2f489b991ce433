// fe_env.hip -- MI355X (gfx950) implementation of the TimeSeriesEnv hot path.
//
// What the reference does with ~660 eager ATen ops and four full-day
// advanced-index copies per step (finenvs/environments/time_series_env.py,
// "TSE", lines 277-536) is ONE kernel launch here:
//
//   phase 1  one lane per (env, asset) account ("sleeve"): action -> share
//            delta, six-stage trade, margin checks, reward, done      TSE:298-421,447-496
//   phase 1b one lane per env: OR of sleeve dones, liquidation fee, reward sum,
//            evaluate-mode bookkeeping, eval-env redraw                TSE:288-289,498-536
//   phase 2  the whole workgroup streams the tile's observations: each wavefront
//            loads 32-byte (O,H,L,C log-return) tuples of the (W, 4A) window from
//            the L2/MALL-resident table with coalesced 16-byte loads, lays them
//            out as 5-tuples (+ position feature) in a wave-private LDS image,
//            reads the image back linearly (ds_read_b128) and writes the
//            (W, 5A) observation as full 1-KiB-per-instruction stores  TSE:423-445
//
// A workgroup (256 threads = 4 wavefronts of 64) owns a TILE of EB consecutive
// envs; tiles are grid-strided.  The observation of a tile is one contiguous
// region of HBM, so phase 2 is a flat, perfectly coalesced store stream.
// Round-2 structure (measurements: DESIGN.md section 5, profiles/r02_microbench/):
// workgroup barriers order LDS only (no store drain), observation stores are
// write-through (sc1, single asset) or non-temporal (multi asset) so that state
// and tables stay in L2, a single-asset tile is a whole number of workgroup
// iterations with 4 (f64) / 6 (f32) workgroups per CU, and the first tile's table
// loads are issued before its accounting.
//
// One translation unit, these files:
//   fe_device_common.h    constants / build knobs, Params, Philox, sleeve accounting, LDS tile layout, input loads
//   fe_store_policy.h     host only: which launches of a large single-asset env stream past the Infinity Cache
//   fe_step_kernel.h      fe_env_kernel (the fused step and reset() rendering)
//   fe_rollout_kernels.h  K-step fused rollouts with an in-kernel policy: linear window / table form, MLP head (MFMA)
//   fe_activations.h      exact-operation sigmoid / tanh shared by the LSTM and MLP heads
//   fe_mlp_head_kernels.h  the MLP head's training entries: device packing, sampled rollout, value on descriptors, backward
//   fe_mlp2_head_kernels.h the two-hidden-layer MLP head: sampled rollout, value on descriptors, backward
//   fe_lstm_kernel.h      K-step fused rollout with the reference's LSTM actor (MFMA), and with the SAC actor's head
//   fe_lstm_rollout_body.h  the register-resident rollout's body, included by both of those kernels
//   fe_lstm_stream_tile.h   one row-tile group of the streamed recurrence at H = 256 / 512 / 1024, included by the large-H
//                           rollout kernel and by fe_lstm_stream_sgrad_body.h
//   fe_lstm_stream_sgrad_body.h  the tile loop of the streamed head's and the streamed critics' recurrence kernels
//   fe_aux_kernels.h      descriptor / render kernels, init kernels (log-returns, day tables), trajectory kernels
//   fe_replay_kernels.h   off-policy replay ring of observation descriptors: append, fused minibatch sample
//   fe_ring_draw_kernels.h  a mini-batch drawn and gathered from the ring's device cursor (capturable updates)
//   fe_ppo_kernels.h     PPO's mini-batch drawn from a keyed permutation and gathered, and its two losses with gradients
//   fe_critic_kernels.h   twin LSTM critics (SAC / TD3) on the rollout body's recurrence, and their Bellman-target epilogue
//   fe_bptt_tile.h            the stages of one backward-through-time tile that the three backward passes below share
//   fe_critic_grad_kernels.h  the twin critics' backward pass through time and its deterministic reduction
//   fe_sac_grad_kernels.h     the SAC actor's backward pass (tanh-Gaussian head, last layer, recurrence) and its reduction
//   fe_lstm_grad_kernels.h    the one-output LSTM head's backward pass (PPO actor / critic, TD3 actor) and its reduction
//   fe_critic_streamed_kernels.h  the twin critics at H = 256 / 512 / 1024: streamed values, targets and backward pass
//   fe_sac_streamed_kernels.h     the SAC actor at H = 256 / 512 / 1024: acting, forward and backward pass (streamed)
//   fe_env.hip            (this file) host side: launch helpers (compile-time dispatch, launch epilogue, rollout
//                         geometry, big-LDS launches), launch geometry of the step, the env object, the C ABI of the
//                         headers in include/
//
// Arithmetic contract: every (float)/(double) cast is a rounding point of the
// reference's mixed f32/f64 tensor arithmetic; this file
// must be compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <new>
#include <numeric>
#include <type_traits>

#include "finenvs_amd.h"
#include "finenvs_amd_ext.h"
#include "finenvs_amd_replay.h"
#include "finenvs_amd_sac.h"
#include "finenvs_amd_critic.h"
#include "finenvs_amd_critic_grad.h"
#include "finenvs_amd_sac_grad.h"
#include "finenvs_amd_lstm_grad.h"
#include "finenvs_amd_lstm_grad_streamed.h"
#include "finenvs_amd_critic_streamed.h"
#include "finenvs_amd_sac_streamed.h"
#include "finenvs_amd_optim.h"
#include "finenvs_amd_replay_cursor.h"
#include "finenvs_amd_ppo.h"
#include "finenvs_amd_mlp_head.h"
#include "finenvs_amd_mlp2_head.h"

#include "fe_device_common.h"
#include "fe_store_policy.h"
#include "fe_step_kernel.h"
#include "fe_rollout_kernels.h"
#include "fe_mlp_head_kernels.h"
#include "fe_mlp2_head_kernels.h"
#include "fe_lstm_kernel.h"
#include "fe_aux_kernels.h"
#include "fe_replay_kernels.h"
#include "fe_ring_draw_kernels.h"
#include "fe_ppo_kernels.h"
#include "fe_critic_kernels.h"
#include "fe_critic_grad_kernels.h"
#include "fe_sac_grad_kernels.h"
#include "fe_lstm_grad_kernels.h"
#include "fe_lstm_grad_streamed_kernels.h"
#include "fe_critic_streamed_kernels.h"
#include "fe_sac_streamed_kernels.h"
#include "fe_optim_kernels.h"

namespace {

// Largest grid of the grid-strided element-wise launches and of the tile-looping rollouts.
constexpr int64_t kMaxGrid = 8 * 256;
// Dynamic LDS a workgroup can have: the MLP and split-LSTM launches refuse more, each with its own message.
constexpr size_t kMaxLds = 160 * 1024;

int64_t capped_grid(int64_t tiles) { return tiles < kMaxGrid ? tiles : kMaxGrid; }

int grid_for(int64_t work_items) {
    const int64_t g = (work_items + kBlock - 1) / kBlock;
    return (int)(g < 1 ? 1 : capped_grid(g));
}

// Observation elements per 16-byte store: the widest that divides an env's observation (1 when its size is odd).
int vec_width(int64_t env_elems, int elem_bytes) {
    int vec = 16 / elem_bytes;
    while (vec > 1 && env_elems % vec != 0) vec /= 2;
    return vec;
}

// Compile-time dispatch.  with_bool calls f(std::true_type) or f(std::false_type); with_layout calls f(OT{}, VEC) for the
// observation layouts that exist (float x 4 / 2 / 1, double x 2 / 1), VEC a std::integral_constant.  Callers name the
// instantiation as kernel<decltype(ot), decltype(V)::value, decltype(S)::value>: only the templates a call site names get
// instantiated.
template <class F>
auto with_bool(bool b, F &&f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// with_nt calls f(std::integral_constant<int, NT>) for the kernels' NT template argument, NT = H / 32 row tiles at
// H = 32 / 64 / 128 (the caller has refused every other H); with_nt<64, 4> serves the streamed kernels, NT = H / 64 at
// H = 256 / 512 / 1024.  The three-argument form composes it with with_bool for kernel<SINGLE, NT>: f(S, NT).
template <int UNIT = 32, int NT0 = 1, class F>
auto with_nt(int32_t H, F &&f) {
    return H == NT0 * UNIT ? f(std::integral_constant<int, NT0>{})
                           : (H == 2 * NT0 * UNIT ? f(std::integral_constant<int, 2 * NT0>{}) : f(std::integral_constant<int, 4 * NT0>{}));
}

template <int UNIT = 32, int NT0 = 1, class F>
auto with_nt(bool single, int32_t H, F &&f) {
    return with_bool(single, [&](auto S) { return with_nt<UNIT, NT0>(H, [&](auto NT) { return f(S, NT); }); });
}

template <class F>
auto with_layout(bool f32, int vec, F &&f) {
    using V1 = std::integral_constant<int, 1>;
    using V2 = std::integral_constant<int, 2>;
    if (f32) return vec == 4 ? f(float{}, std::integral_constant<int, 4>{}) : (vec == 2 ? f(float{}, V2{}) : f(float{}, V1{}));
    return vec == 2 ? f(double{}, V2{}) : f(double{}, V1{});
}

// The launch epilogue: FE_OK, or FE_ERR_HIP with "<who> launch: <HIP error>".  `he` is what hipLaunchKernel returned; after
// hipLaunchKernelGGL, which returns nothing, the one-argument form asks hipGetLastError.
int launched(const char *who, hipError_t he) {
    return he == hipSuccess ? FE_OK : fail(FE_ERR_HIP, "%s launch: %s", who, hipGetErrorString(he));
}

int launched(const char *who) { return launched(who, hipGetLastError()); }

// ... of stage `what` of entry `who`: reported as "<who>: <what> launch: <HIP error>"
int launched(const char *who, const char *what, hipError_t he = hipGetLastError()) {
    char step[96];
    snprintf(step, sizeof(step), "%s: %s", who, what);
    return launched(step, he);
}

}  // namespace

struct fe_env {
    fe_config cfg;
    Params p;
    int grid;
    int vec;  // observation elements per 16-byte store (1 when the env size is odd)
    size_t lds;
    size_t lds_promoted;  // dynamic LDS of the kernel fe_env_step_promoted dispatches to (== lds unless it takes the tile loop at A = 1)
    bool promoted_used;   // sticky: fe_env_step_promoted has been called (fe_env_launch_info then describes that kernel)
    // the observation buffer that may live in the Infinity Cache: the store policy is decided per launch from how the
    // buffers are actually used (launch_env, fe_store_policy.h).  Relaxed atomics: a stale value costs one launch the other
    // policy, never correctness.
    mutable FeObsResidency obs_residency;
    bool bound;
    int cus;              // compute units of that device
    int tile_override, grid_override, rollout_tile_override;  // fe_env_set_launch (tuning), 0 = automatic
    int device;           // HIP device the tables live on; every launch runs there
    double *owned_logret; // log-return table computed by fe_env_create(logret = NULL), else null
    unsigned int *ticket; // evaluate mode: 4 bytes of device memory for the notify form's last-workgroup detection
};

// Makes the env's device current for the duration of a call and restores the caller's device
// afterwards: the reference's `device_id` argument works without torch.cuda.set_device (TSE:28, 45),
// so a process driving several envs on several GPUs must not have to juggle the current device.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        if (device < 0) {
            err = hipErrorInvalidDevicePointer;
            return;
        }
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) {
            err = hipSetDevice(device);
            switched = err == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    // The device prologue of an entry point: `if (int rc = guard.status()) return rc;`
    int status(const char *what = "hipSetDevice") const { return err == hipSuccess ? FE_OK : hip_fail(err, what); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// Device a caller-owned pointer lives on (-1 if it is not device memory).
static int device_of(const void *ptr) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    if (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged) return -1;
    return attr.device;
}

static int require_bound(const fe_env *env, const char *who) {
    return env->bound ? FE_OK : fail(FE_ERR_STATE, "%s: state not bound", who);
}

// Frees what fe_env_create allocated, and the env; the env's device is current.
static void release_env(fe_env *env) {
    if (env->owned_logret) (void)hipFree(env->owned_logret);
    if (env->ticket) (void)hipFree(env->ticket);
    delete env;
}

// Host-side preparation of kernels with more than the default 64 KiB of dynamic LDS, done once instead of per call:
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per (device, function) and monotone here (only ever raised, so
// envs with different sizes cannot undercut each other), the occupancy query is cached per (device, function, block,
// LDS).  At small env counts the fused rollouts are host-bound: the two runtime calls cost as much as a launch
// (profiles/r03_microbench/host_prep_cache.txt).
struct LaunchPrep {
    int device;
    const void *kern;
    int block;
    size_t lds_max;      // largest dynamic LDS size set for (device, kern) so far
    size_t occ_lds;      // the LDS size the cached occupancy answer belongs to
    int occ_per_cu;      // 0 = not asked yet
};
static LaunchPrep g_prep[64];
static int g_nprep = 0;
static pthread_mutex_t g_prep_mu = PTHREAD_MUTEX_INITIALIZER;

// Makes `kern` launchable with `lds` bytes of dynamic LDS on `device` and, if per_cu != null, returns how many
// `block`-thread workgroups of it fit a CU.  The caller has made `device` current.
static hipError_t prepare_kernel(int device, const void *kern, int block, size_t lds, int *per_cu) {
    pthread_mutex_lock(&g_prep_mu);
    LaunchPrep *e = nullptr;
    for (int i = 0; i < g_nprep; ++i)
        if (g_prep[i].device == device && g_prep[i].kern == kern && g_prep[i].block == block) e = &g_prep[i];
    if (!e && g_nprep < (int)(sizeof(g_prep) / sizeof(g_prep[0]))) {
        e = &g_prep[g_nprep++];
        *e = LaunchPrep{device, kern, block, 0, 0, 0};
    }
    LaunchPrep local{device, kern, block, 0, 0, 0};
    if (!e) e = &local;  // table full: behave as before (per call)
    hipError_t he = hipSuccess;
    if (lds > e->lds_max) {
        he = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (he == hipSuccess) e->lds_max = lds;
    }
    if (he == hipSuccess && per_cu) {
        if (e->occ_per_cu == 0 || e->occ_lds != lds) {
            int n = 0;
            he = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, block, lds);
            if (he == hipSuccess) {
                e->occ_per_cu = n < 1 ? 1 : n;
                e->occ_lds = lds;
            }
        }
        *per_cu = e->occ_per_cu;
    }
    pthread_mutex_unlock(&g_prep_mu);
    return he;
}

// The big-LDS path of the MLP and split-LSTM rollouts (the caller has refused lds > kMaxLds in its own words):
// prepare_kernel for a kBlock-thread launch, its failure reported as "<who>: hipFuncSetAttribute: <HIP error>" ...
static int prepare_big_lds(int device, const void *kern, size_t lds, const char *who) {
    const hipError_t he = prepare_kernel(device, kern, kBlock, lds, nullptr);
    return he == hipSuccess ? FE_OK : fail(FE_ERR_HIP, "%s: hipFuncSetAttribute: %s", who, hipGetErrorString(he));
}

// ... then the launch of a kernel that takes (Params, its argument block).
template <class Args>
static int launch_big_lds(int device, const void *kern, int64_t grid, size_t lds, Params &p, Args &r, void *stream,
                          const char *who) {
    if (int rc = prepare_big_lds(device, kern, lds, who)) return rc;
    void *args[] = {&p, &r};
    return launched(who, hipLaunchKernel(kern, dim3((unsigned)grid), dim3(kBlock), args, lds, (hipStream_t)stream));
}

// Tile geometry of the fused rollouts that keep one workgroup per tile (linear, table, MLP, split-LSTM accounting): state
// lives in HBM between steps but every tile is revisited by the same workgroup, so a grid of one workgroup per tile
// (capped) keeps the K-step loop entirely inside the launch.  `eb` is the rollout's own tile, at most kBlock / A sleeves.
// fe_env_set_launch(rollout_tile_envs) either replaces it (`replace`: linear, MLP) or may only shrink it (table, split
// LSTM).  Sets p.EB and p.num_tiles and returns the grid.
static int64_t rollout_geometry(const fe_env *env, Params &p, int64_t eb, bool replace) {
    const int64_t cap = kBlock / p.A > 0 ? kBlock / p.A : 1;
    if (eb > cap) eb = cap;
    const int64_t tile_override = env->rollout_tile_override;
    if (tile_override > 0 && (replace || tile_override < eb)) eb = tile_override < cap ? tile_override : cap;
    p.EB = (int)eb;
    p.num_tiles = (p.N + eb - 1) / eb;
    return capped_grid(p.num_tiles);
}

// The kernel instantiation a given env dispatches to (shared by launch and occupancy query).  FORM (fe_step_kernel.h):
// kFull = the launch has optional outputs (evaluate-mode bookkeeping, episode statistics, trajectory descriptors), kLean =
// none of them (the action copy of fe_env_step_traj is written by every form), kNotify = lean + the host flag of
// fe_env_step_notify; same launch bounds, same LDS.
template <bool RESET_ONLY, int FORM>
static const void *kernel_for(bool f32, int vec, bool single) {
    return with_layout(f32, vec, [=](auto ot, auto V) {
        return with_bool(single, [](auto S) {
            return (const void *)fe_env_kernel<decltype(ot), decltype(V)::value, decltype(S)::value, RESET_ONLY, FORM>;
        });
    });
}

// fe_env_step_promoted: the step kernel with the promoted arithmetic, full forms only.  `pipelined`: the single-asset
// software pipeline (f64 observations, the reference's dtype); else the tile loop, which serves any A -- single-asset envs
// with f32 observations take it too (the pipeline's f32 instantiation has no registers to spare for f64 actions at its 6
// wavefronts per SIMD: it spilled).
template <int FORM>
static const void *promoted_kernel_for(bool f32, int vec, bool pipelined) {
    return with_layout(f32, vec, [=](auto ot, auto V) {
        using OT = decltype(ot);
        if constexpr (std::is_same<OT, double>::value) {
            if (pipelined) return (const void *)fe_env_promoted_kernel<double, decltype(V)::value, true, FORM>;
        }
        return (const void *)fe_env_promoted_kernel<OT, decltype(V)::value, false, FORM>;
    });
}

// Per-call pointers go into a local copy of the parameter block: the env object itself is not
// modified by reset/step, so concurrent calls on different streams do not race on the host side.
template <bool RESET_ONLY>
static int launch_env(const fe_env *env, const float *actions, void *obs, double *rewards, int32_t *dones,
                      hipStream_t st, int64_t *desc_src = nullptr, double *desc_pos = nullptr, float *act_store = nullptr,
                      uint64_t *host_flag = nullptr, uint64_t flag_seq = 0, int promoted = -1) {
    Params p = env->p;
    p.actions = actions;
    p.act_f64 = promoted == 1 ? 1 : 0;
    p.obs = obs;
    p.rew = rewards;
    p.done = dones;
    p.desc_src = desc_src;
    p.desc_pos = desc_pos;
    p.act_store = act_store;
    p.host_flag = reinterpret_cast<unsigned long long *>(host_flag);
    p.flag_seq = flag_seq;
    p.has_stats = p.run_ret != nullptr ? 1 : 0;
    void *args[] = {&p};
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    const bool f32 = env->cfg.obs_is_f32 != 0, single = p.A == 1;
    // (the action copy alone does not need the full form: every form writes it)
    const bool full = !RESET_ONLY && (p.evaluate || p.run_ret || desc_src);
    const void *kern = RESET_ONLY ? kernel_for<true, kLean>(f32, env->vec, single)
                       : (host_flag ? (full ? kernel_for<false, kFullNotify>(f32, env->vec, single) : kernel_for<false, kNotify>(f32, env->vec, single))
                                    : (full ? kernel_for<false, kFull>(f32, env->vec, single) : kernel_for<false, kLean>(f32, env->vec, single)));
    size_t lds = env->lds;
    if (!RESET_ONLY && promoted >= 0) {
        const bool pipelined = single && !f32;
        kern = host_flag ? promoted_kernel_for<kFullNotify>(f32, env->vec, pipelined) : promoted_kernel_for<kFull>(f32, env->vec, pipelined);
        lds = env->lds_promoted;
    }
    if (!RESET_ONLY) {
        // Store policy of a large single-asset observation (Params::obs_stream, fe_device_common.h): sc1 | nt keeps the
        // stream out of the 256 MiB Infinity Cache, which pays when the caller goes round buffers that together overflow
        // it (a ring of two, fresh tensors per call) -- but ONE buffer of 128 - 256 MiB that is rewritten again and again
        // is absorbed by the cache and runs 3 % faster with plain sc1 (profiles/r04_microbench/ring_alternation.txt: 27.5
        // vs 28.4 us), also while the other ring members stream past it (profiles/launch_head/ab.txt).  So the env keeps
        // one resident buffer: launches that write it store plain, all others stream (fe_obs_store_policy).
        if (p.obs_stream) p.obs_stream = fe_obs_store_policy(env->obs_residency, obs, (uint64_t)p.N * p.env_elems * (f32 ? 4 : 8));
    }
    return launched(RESET_ONLY ? "fe_env_reset_obs" : "fe_env_step", hipLaunchKernel(kern, dim3(env->grid), dim3(kBlock), args, lds, st));
}

// The step entry points: their shared checks, then the launch.  `who` names the entry point.  Every form is
// fe_env_step_promoted with f32 actions (actions_are_f64 = 0: its two f64 checks pass) except for the kernel choice,
// `promoted`.  host_flag != null (a notify form) needs the eval env on this shard.
static int step_checked(fe_env *env, const char *who, bool promoted, const void *actions, int32_t actions_are_f64, void *obs,
                        double *rewards, int32_t *dones, float *actions_store_out, int64_t *obs_src_out, double *obs_pos_out,
                        uint64_t *host_flag, uint64_t seq, void *stream) {
    if (!env || !actions || !obs || !rewards || !dones) return fail(FE_ERR_ARG, "%s: null argument", who);
    if (actions_are_f64 != 0 && actions_are_f64 != 1) return fail(FE_ERR_ARG, "%s: actions_are_f64 must be 0 or 1", who);
    if ((obs_src_out == nullptr) != (obs_pos_out == nullptr))
        return fail(FE_ERR_ARG, "%s: obs_src_out and obs_pos_out go together", who);
    if (actions_store_out && actions_are_f64)
        return fail(FE_ERR_ARG, "%s: actions_store_out is an f32 copy; f64 actions have none", who);
    if (actions_store_out == actions) actions_store_out = nullptr;  // already where they belong
    if (int rc = require_bound(env, who)) return rc;
    if (host_flag && env->p.eval_env < 0 && !env->cfg.evaluate)
        return fail(FE_ERR_ARG, "%s: this training-mode env has no evaluation env (a shard that does not own it)", who);
    if (promoted) env->promoted_used = true;
    return launch_env<false>(env, reinterpret_cast<const float *>(actions), obs, rewards, dones, (hipStream_t)stream, obs_src_out,
                             obs_pos_out, actions_store_out, host_flag, seq, promoted ? actions_are_f64 : -1);
}

// Launch geometry of the step / reset kernels: tile size EB, tile count, grid, dynamic LDS.
static int configure_launch(fe_env *env) {
    const fe_config &cfg = env->cfg;
    const int A = cfg.A;
    const void *kern = kernel_for<false, kFull>(cfg.obs_is_f32 != 0, env->vec, A == 1);
    // How many workgroups the chip holds at once for this kernel variant (registers + LDS).
    int64_t cap = kBlock / A > 0 ? kBlock / A : 1;  // one sleeve per lane in phase 1
    int per_cu = 0;
    hipError_t he = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kBlock, lds_bytes((int)cap, A));
    if (he != hipSuccess) return hip_fail(he, "hipOccupancyMaxActiveBlocksPerMultiprocessor");
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 8) per_cu = 8;
    int64_t resident = (int64_t)env->cus * per_cu;
    if (resident > 8) resident -= resident % 8;  // keeps tile % 8 (the XCD label) constant per workgroup
    // Tile = EB consecutive envs.  Aim for ~8/3 tiles per resident workgroup: measured on
    // MI355X (round 1, profiles/r01_microbench/sweep_c2.txt, 64k envs) a few short tiles per workgroup beat one long
    // tile (workgroups drift apart, so phase 1 of one hides under phase 2 of its CU-mates).
    int64_t EB = (3 * cfg.N + 4 * resident) / (8 * resident);
    if (EB < 1) EB = 1;
    if (EB > cap) EB = cap;
    int wgs_per_cu = 0;  // 0 = whatever the occupancy query allows
    if (A == 1) {
        // Single-asset envs (measured at 64k envs x W64 on a shared observation ring, tools/ab_step.py,
        // profiles/r02_microbench/sweep{3,4}_c2.txt, sweep_f32_c2.txt).  A tile must be a whole number of workgroup
        // iterations of phase 2 (4 wavefronts x one 5-KiB image = 512 f64 / 1024 f32 tuples): with f64 observations
        // 8 envs of W = 64 run 31.2 us, 12 envs 35.2 us, 6 envs 42.2 us.  Fewer workgroups than the occupancy limit
        // start faster (the dispatch ramp of 1792 workgroups costs up to 5 us of a 31 us launch): f64 observations
        // are fastest with 4 workgroups per CU and ~8 short tiles each (31.2-31.8 us vs 33.0-34.2 us for the round-1
        // geometry), f32 observations (half the bytes, a 17-19 us launch) with 6 per CU and 1-2 longer tiles each
        // (17.4 us vs 19.4 us).
        const int64_t wg_tuples = 4 * (kStageBytes / (5 * (cfg.obs_is_f32 ? 4 : 8)));
        const int64_t unit = wg_tuples / std::gcd(wg_tuples, (int64_t)cfg.W);  // envs per whole workgroup iteration
        if (unit <= cap) {
            wgs_per_cu = cfg.obs_is_f32 ? (env->vec == 4 ? kF32StepWaves<float, 4> : kF32StepWaves<float, 1>) : 4;
            const int64_t res = (int64_t)env->cus * wgs_per_cu;
            if (resident > res) resident = res;
            // tiles per workgroup aimed at: 8 (f64) resp. 4/3 (f32)
            const int64_t num = cfg.obs_is_f32 ? 3 * cfg.N : cfg.N, den = (cfg.obs_is_f32 ? 4 : 8) * resident * unit;
            int64_t m = (num + den / 2) / den;
            if (m < 1) m = 1;
            EB = unit * m;
            if (EB > cap) EB = cap - cap % unit;
        }
    }
    if (env->tile_override > 0) EB = env->tile_override < cap ? env->tile_override : cap;
    const int64_t num_tiles = (cfg.N + EB - 1) / EB;
    // the LDS footprint depends on EB: ask again with the real size before fixing the grid
    he = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kBlock, lds_bytes((int)EB, A));
    if (he == hipSuccess && per_cu >= 1) {
        if (per_cu > 8) per_cu = 8;
        if (wgs_per_cu > 0 && per_cu > wgs_per_cu) per_cu = wgs_per_cu;  // see above
        resident = (int64_t)env->cus * per_cu;
        if (resident > 8) resident -= resident % 8;
    }
    int64_t grid = num_tiles < resident ? num_tiles : resident;
    if (A > 1) {
        // Multi-asset envs launch k x the resident workgroup count (k = 8, 4 or 2; every workgroup still walks >= 2 tiles, grid-strided):
        // the hardware hands the later workgroups out in order as earlier ones retire, so the launch is balanced by dispatch instead of
        // by a fixed share per persistent workgroup, whose shares of HBM differ by 10x (profiles/r06_microbench/config3_launch_size.md).
        // Measured (round 6, interleaved on one ring where it fits; table 11 there): k = 8 against k = 1 -- config 4 25.59 -> 24.00 ms
        // (6.29 -> 6.71 TB/s of observation: torch's fill rate on that buffer), config-5 shard 13.03 -> 12.59 ms, config 3 3.62 -> 3.53 ms;
        // multiples of the resident count only (4 096 / 8 192 of 1 536 resident: no gain at config 3), and not one tile per
        // workgroup (k = 64 at config 4: 2 % slower than k = 1).  The tile % 8 = XCD mapping is unchanged (k x resident is a multiple of 8).
        // Single-asset envs keep the resident grid: there every larger grid measured slower (4 - 57 %, their launch is 28 us).
        for (int k = 8; k > 1; k >>= 1) {
            if ((int64_t)k * resident <= num_tiles / 2) {
                grid = (int64_t)k * resident;
                break;
            }
        }
    }
    if (env->grid_override > 0) grid = env->grid_override;
    env->grid = (int)grid;
    env->lds = lds_bytes((int)EB, A);
    // (fe_env_step_promoted: single-asset envs with f32 observations take the tile loop, which keeps per-sleeve arrays in LDS)
    env->lds_promoted = (A == 1 && cfg.obs_is_f32 == 0) ? env->lds : lds_bytes((int)EB, A, /*per_sleeve_arrays=*/true);
    env->p.EB = (int)EB;
    env->p.num_tiles = num_tiles;
    return FE_OK;
}


// fe_env_create past its argument checks, with the env's device current: the device allocations, the launch geometry and
// the parameter block.  On failure the caller releases the env.
static int init_env(fe_env *env, const double *prices, const double *logret, int cus) {
    const fe_config *cfg = &env->cfg;
    hipError_t he;
    if (cfg->evaluate) {
        if ((he = hipMalloc(&env->ticket, sizeof(unsigned int))) != hipSuccess || (he = hipMemset(env->ticket, 0, sizeof(unsigned int))) != hipSuccess)
            return hip_fail(he, "fe_env_create: hipMalloc(ticket)");
    }
    if (!logret) {
        // logret = NULL: compute the table from the prices (the one allocation this library owns)
        const int64_t tuples = cfg->D * cfg->L * (int64_t)cfg->A;
        if ((he = hipMalloc(&env->owned_logret, (size_t)tuples * 32)) != hipSuccess) return hip_fail(he, "fe_env_create: hipMalloc(logret)");
        hipLaunchKernelGGL(fe_logret_tables_kernel, dim3(grid_for(tuples)), dim3(kBlock), 0, (hipStream_t) nullptr,
                           prices, env->owned_logret, cfg->D, cfg->L, cfg->A);
        he = hipGetLastError();
        if (he == hipSuccess) he = hipStreamSynchronize(nullptr);
        if (he != hipSuccess) return hip_fail(he, "fe_env_create: log-return table");
        logret = env->owned_logret;
    }
    const int A = cfg->A;
    const int64_t env_elems = (int64_t)cfg->W * 5 * cfg->A;
    env->vec = vec_width(env_elems, cfg->obs_is_f32 ? 4 : 8);
    env->cus = cus;
    Params &p = env->p;
    p.N = cfg->N;
    p.A = A;
    if (int rc = configure_launch(env)) return rc;
    p.ticket = env->ticket;
    p.P = prices;
    p.LR = logret;
    p.N = cfg->N; p.D = cfg->D; p.L = cfg->L;
    p.W = cfg->W; p.A = A;
    p.eval_env = cfg->evaluate ? -1 : cfg->eval_env;
    p.seed = cfg->seed;
    p.evaluate = cfg->evaluate ? 1 : 0;
    p.redraw_mode = cfg->redraw_mode;
    p.env_elems = (uint32_t)env_elems;
    // One observation buffer of 128 MiB or more: a ring of two (or the allocator's recycled blocks behind fresh tensors)
    // overflows the 256 MiB Infinity Cache, and the store stream is better kept out of it (fe_device_common.h, store policy)
    p.obs_stream = cfg->A == 1 && cfg->N * env_elems * (cfg->obs_is_f32 ? 4 : 8) >= (128ll << 20) ? 1 : 0;
    p.div_WA = make_fastdiv((uint32_t)((int64_t)cfg->W * cfg->A));
    p.div_A = make_fastdiv((uint32_t)A);
    p.scale32 = (float)((double)cfg->max_shares + 0.5);
    p.scale64 = (double)cfg->max_shares + 0.5;
    p.ms64 = (double)cfg->max_shares;
    p.ms32 = (float)cfg->max_shares;
    p.c32 = (float)cfg->commission;
    p.imr32 = (float)cfg->init_margin;
    p.S32 = (float)cfg->starting_balance;
    p.comm = cfg->commission;
    p.imr = cfg->init_margin;
    p.one_mmr = 1.0 + cfg->maint_margin;
    p.S = cfg->starting_balance;
    return FE_OK;
}

// The six gradients of one LSTM and its one-output layer, fe_lstm_grads or fe_critic_grads (templates: outside the
// extern "C" block): every pointer is there ...
template <class Grads>
static bool head_grads_given(const Grads *g) {
    return g && g->w_ih && g->w_hh && g->b_ih && g->b_hh && g->w_out && g->b_out;
}

// ... and into g_wih ... g_bout of a kernel's argument block.
template <class Args, class Grads>
static void head_grads_into(Args &g, const Grads &s) {
    g.g_wih = s.w_ih; g.g_whh = s.w_hh; g.g_bih = s.b_ih; g.g_bhh = s.b_hh; g.g_wout = s.w_out; g.g_bout = s.b_out;
}

extern "C" {

int fe_version(void) { return FE_ABI_VERSION; }

const char *fe_last_error(void) { return g_err; }

int fe_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int fe_env_create(const fe_config *cfg, const double *prices, const double *logret, fe_env **out) {
    if (!cfg || !out) return fail(FE_ERR_ARG, "fe_env_create: null argument");
    if (!prices) return fail(FE_ERR_ARG, "fe_env_create: the price table is required");
    if (cfg->N < 1 || cfg->D < 1) return fail(FE_ERR_ARG, "fe_env_create: N=%lld D=%lld must be >= 1", (long long)cfg->N, (long long)cfg->D);
    if (cfg->W < 1 || cfg->L <= cfg->W)
        return fail(FE_ERR_ARG, "fe_env_create: need 1 <= W < L (W=%lld, L=%lld)", (long long)cfg->W, (long long)cfg->L);
    if (cfg->A < 1 || cfg->A > FE_MAX_ASSETS)
        return fail(FE_ERR_ARG, "fe_env_create: A=%lld outside 1..%lld", (long long)cfg->A, (long long)FE_MAX_ASSETS);
    if (cfg->max_shares < 0) return fail(FE_ERR_ARG, "fe_env_create: max_shares < 0");
    if (cfg->redraw_mode != 0 && cfg->redraw_mode != 1) return fail(FE_ERR_ARG, "fe_env_create: redraw_mode must be 0 or 1");
    if (cfg->eval_env >= cfg->N) return fail(FE_ERR_ARG, "fe_env_create: eval_env out of range");
    if ((int64_t)cfg->W * 5 * cfg->A > (1ll << 24)) return fail(FE_ERR_ARG, "fe_env_create: W*5*A too large");
    int ndev = 0;
    hipError_t he = hipGetDeviceCount(&ndev);
    if (he != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        return fail(FE_ERR_HIP, "fe_env_create: no HIP device (this library has no CPU path)");
    }
    // the env lives where its tables live, whatever the caller's current device is
    const int dev = device_of(prices);
    if (dev < 0 || dev >= ndev) return fail(FE_ERR_ARG, "fe_env_create: prices is not a device pointer");
    if (logret && device_of(logret) != dev)
        return fail(FE_ERR_ARG, "fe_env_create: prices and logret live on different devices");
    DeviceGuard guard(dev);
    if (int rc = guard.status()) return rc;
    hipDeviceProp_t prop;
    if ((he = hipGetDeviceProperties(&prop, dev)) != hipSuccess) return hip_fail(he, "hipGetDeviceProperties");

    fe_env *env = new (std::nothrow) fe_env();  // value-initialized: every field starts zero / null
    if (!env) return fail(FE_ERR_ARG, "fe_env_create: out of host memory");
    env->cfg = *cfg;
    env->device = dev;
    if (int rc = init_env(env, prices, logret, prop.multiProcessorCount)) {
        release_env(env);
        return rc;
    }
    *out = env;
    return FE_OK;
}

int fe_env_bind_state(fe_env *env, int64_t *env_idx, int64_t *spot0, float *cash, float *long_shares,
                      float *short_shares, double *margin, uint8_t *terminated, float *episode_returns,
                      int64_t *counters) {
    if (!env) return fail(FE_ERR_ARG, "fe_env_bind_state: null env");
    if (!env_idx || !spot0 || !cash || !long_shares || !short_shares || !margin || !counters)
        return fail(FE_ERR_ARG, "fe_env_bind_state: null state pointer");
    if (env->cfg.evaluate && (!terminated || !episode_returns))
        return fail(FE_ERR_ARG, "fe_env_bind_state: evaluate mode needs terminated and episode_returns");
    Params &p = env->p;
    p.env_idx = env_idx; p.spot0 = spot0; p.cash = cash; p.lng = long_shares; p.sht = short_shares;
    p.margin = margin; p.terminated = terminated; p.ep_ret = episode_returns;
    p.counters = reinterpret_cast<unsigned long long *>(counters);
    env->bound = true;
    return FE_OK;
}

int fe_env_bind_f32_table(fe_env *env, const float *logret_f32) {
    if (!env) return fail(FE_ERR_ARG, "fe_env_bind_f32_table: null env");
    if (logret_f32 && !env->cfg.obs_is_f32)
        return fail(FE_ERR_ARG, "fe_env_bind_f32_table: only meaningful with f32 observations");
    env->p.LR32 = logret_f32;
    return FE_OK;
}

int fe_env_bind_stats(fe_env *env, float *running_returns, double *accumulators, float *eval_return) {
    if (!env) return fail(FE_ERR_ARG, "fe_env_bind_stats: null env");
    if (!running_returns) {  // unbind
        env->p.run_ret = nullptr;
        env->p.stat_acc = nullptr;
        env->p.stat_eval = nullptr;
        return FE_OK;
    }
    if (!accumulators || !eval_return) return fail(FE_ERR_ARG, "fe_env_bind_stats: null accumulator pointer");
    env->p.run_ret = running_returns;
    env->p.stat_acc = accumulators;
    env->p.stat_eval = eval_return;
    return FE_OK;
}

int fe_env_stats_reduce(fe_env *env, double *out, void *stream) {
    if (!env || !out) return fail(FE_ERR_ARG, "fe_env_stats_reduce: null argument");
    if (!env->p.stat_acc) return fail(FE_ERR_STATE, "fe_env_stats_reduce: no statistics bound (fe_env_bind_stats)");
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    hipLaunchKernelGGL(fe_stats_reduce_kernel, dim3(1), dim3(kStatsLanes), 0, (hipStream_t)stream, env->p.stat_acc, env->p.N, out);
    return launched("fe_env_stats_reduce");
}

int fe_env_reset_obs(fe_env *env, void *obs, void *stream) {
    if (!env || !obs) return fail(FE_ERR_ARG, "fe_env_reset_obs: null argument");
    if (int rc = require_bound(env, "fe_env_reset_obs")) return rc;
    return launch_env<true>(env, nullptr, obs, nullptr, nullptr, (hipStream_t)stream);
}

int fe_env_step(fe_env *env, const float *actions, void *obs, double *rewards, int32_t *dones, void *stream) {
    return step_checked(env, "fe_env_step", false, actions, 0, obs, rewards, dones, nullptr, nullptr, nullptr, nullptr, 0, stream);
}

int fe_env_step_notify(fe_env *env, const float *actions, void *obs, double *rewards, int32_t *dones,
                       uint64_t *host_flag, uint64_t seq, void *stream) {
    if (!host_flag) return fail(FE_ERR_ARG, "fe_env_step_notify: null argument");
    return step_checked(env, "fe_env_step_notify", false, actions, 0, obs, rewards, dones, nullptr, nullptr, nullptr, host_flag, seq,
                        stream);
}

int fe_env_step_traj_notify(fe_env *env, const float *actions, void *obs, double *rewards, int32_t *dones,
                            float *actions_store_out, int64_t *obs_src_out, double *obs_pos_out, uint64_t *host_flag,
                            uint64_t seq, void *stream) {
    if (!host_flag) return fail(FE_ERR_ARG, "fe_env_step_traj_notify: null argument");
    return step_checked(env, "fe_env_step_traj_notify", false, actions, 0, obs, rewards, dones, actions_store_out, obs_src_out,
                        obs_pos_out, host_flag, seq, stream);
}

int fe_env_step_promoted(fe_env *env, const void *actions, int32_t actions_are_f64, void *obs, double *rewards,
                         int32_t *dones, float *actions_store_out, int64_t *obs_src_out, double *obs_pos_out,
                         uint64_t *host_flag, uint64_t seq, void *stream) {
    return step_checked(env, "fe_env_step_promoted", true, actions, actions_are_f64, obs, rewards, dones, actions_store_out,
                        obs_src_out, obs_pos_out, host_flag, seq, stream);
}

int fe_host_flag_create(uint64_t **host_flag) {
    if (!host_flag) return fail(FE_ERR_ARG, "fe_host_flag_create: null argument");
    void *ptr = nullptr;
    // mapped into the device's address space, coherent (fine-grained): a device store is visible to a polling host thread
    hipError_t he = hipHostMalloc(&ptr, sizeof(uint64_t), hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable);
    if (he != hipSuccess) return hip_fail(he, "fe_host_flag_create: hipHostMalloc");
    *reinterpret_cast<volatile uint64_t *>(ptr) = 0;
    *host_flag = reinterpret_cast<uint64_t *>(ptr);
    return FE_OK;
}

int fe_host_flag_destroy(uint64_t *host_flag) {
    if (host_flag) (void)hipHostFree(host_flag);
    return FE_OK;
}

int fe_env_step_traj(fe_env *env, const float *actions, void *obs, double *rewards, int32_t *dones,
                     float *actions_store_out, int64_t *obs_src_out, double *obs_pos_out, void *stream) {
    return step_checked(env, "fe_env_step_traj", false, actions, 0, obs, rewards, dones, actions_store_out, obs_src_out,
                        obs_pos_out, nullptr, 0, stream);
}

int fe_env_describe(fe_env *env, int64_t *obs_src, double *obs_pos, void *stream) {
    if (!env || !obs_src || !obs_pos) return fail(FE_ERR_ARG, "fe_env_describe: null argument");
    if (int rc = require_bound(env, "fe_env_describe")) return rc;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    const Params &p = env->p;
    dim3 g(grid_for(p.N * p.A)), b(kBlock);
    with_bool(p.A == 1, [&](auto S) {
        hipLaunchKernelGGL(fe_describe_kernel<decltype(S)::value>, g, b, 0, (hipStream_t)stream, p, obs_src, obs_pos);
    });
    return launched("fe_env_describe");
}

int fe_env_render(fe_env *env, const int64_t *obs_src, const double *obs_pos, void *obs, void *stream) {
    if (!env) return fail(FE_ERR_ARG, "fe_env_render: null argument");
    return fe_env_render_n(env, obs_src, obs_pos, env->cfg.N, obs, stream);
}

int fe_env_render_n(fe_env *env, const int64_t *obs_src, const double *obs_pos, int64_t count, void *obs, void *stream) {
    if (!env || !obs_src || !obs_pos || !obs || count < 0) return fail(FE_ERR_ARG, "fe_env_render_n: bad argument");
    if (count == 0) return FE_OK;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    Params p = env->p;
    p.obs = obs;
    p.N = count;  // any number of descriptors, e.g. a minibatch drawn from a trajectory of them
    p.num_tiles = (count + p.EB - 1) / p.EB;
    dim3 g((unsigned)(p.num_tiles < (int64_t)env->grid ? p.num_tiles : (int64_t)env->grid)), b(kBlock);
    with_layout(env->cfg.obs_is_f32 != 0, env->vec, [&](auto ot, auto V) {
        with_bool(p.A == 1, [&](auto S) {
            hipLaunchKernelGGL((fe_render_kernel<decltype(ot), decltype(V)::value, decltype(S)::value>), g, b, env->lds,
                               (hipStream_t)stream, p, obs_src, obs_pos);
        });
    });
    return launched("fe_env_render_n");
}

int fe_env_check_descriptors(fe_env *env, const int64_t *obs_src, int64_t count, int64_t *first_bad, void *stream) {
    if (!env || !obs_src || !first_bad || count < 0) return fail(FE_ERR_ARG, "fe_env_check_descriptors: bad argument");
    *first_bad = -1;
    if (count == 0) return FE_OK;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *d = nullptr, h[2] = {0ull, (unsigned long long)count};
    hipError_t he = hipMalloc(&d, sizeof(h));
    if (he != hipSuccess) return hip_fail(he, "fe_env_check_descriptors: hipMalloc");
    he = hipMemcpyAsync(d, h, sizeof(h), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) {
        const Params &p = env->p;
        hipLaunchKernelGGL(fe_check_descriptors_kernel, dim3(grid_for(count)), dim3(kBlock), 0, st, obs_src, count,
                           4 * (int64_t)p.A, (int64_t)p.W, p.D * p.L, d);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    int64_t bad_value = 0;
    if (he == hipSuccess && h[0] != 0) {
        he = hipMemcpy(&bad_value, obs_src + h[1], sizeof(int64_t), hipMemcpyDeviceToHost);
    }
    (void)hipFree(d);
    if (he != hipSuccess) return hip_fail(he, "fe_env_check_descriptors");
    if (h[0] != 0) {
        *first_bad = (int64_t)h[1];
        return fail(FE_ERR_ARG, "fe_env_check_descriptors: %llu of %lld descriptors lie outside this env's log-return table "
                    "(first: obs_src[%lld] = %lld; valid: multiples of %d with offset / %d + W <= D*L = %lld, W = %d)",
                    h[0], (long long)count, (long long)h[1], (long long)bad_value, 4 * env->p.A, 4 * env->p.A,
                    (long long)(env->p.D * env->p.L), env->p.W);
    }
    return FE_OK;
}

int fe_env_rollout_linear(fe_env *env, const double *weights, double bias, int32_t K, int64_t *obs_src,
                          double *obs_pos, float *actions_out, double *rewards_out, int32_t *dones_out,
                          void *stream) {
    if (!env || !weights || !obs_src || !obs_pos || !rewards_out || !dones_out || K < 1)
        return fail(FE_ERR_ARG, "fe_env_rollout_linear: bad argument");
    if (int rc = require_bound(env, "fe_env_rollout_linear")) return rc;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    Params p = env->p;
    // the rollout is latency-bound (policy -> accounting -> policy ...): 64 sleeves per workgroup measured
    // best at 64k envs (tools/fused_bench.py), independent of the tile the streaming step kernel uses --
    // but never fewer than 8 envs per workgroup when they fit
    const int64_t grid = rollout_geometry(env, p, 64 / p.A > 8 ? 64 / p.A : 8, /*replace=*/true);
    const size_t lds = rollout_lds_bytes(p.EB, p.A, p.W);
    RolloutArgs r;
    r.weights = weights; r.bias = bias; r.K = K; r.obs_src = obs_src; r.obs_pos = obs_pos;
    r.actions_out = actions_out; r.rew_out = rewards_out; r.done_out = dones_out;
    with_bool(p.A == 1, [&](auto S) {
        hipLaunchKernelGGL(fe_rollout_linear_kernel<decltype(S)::value>, dim3((unsigned)grid), dim3(kBlock), lds,
                           (hipStream_t)stream, p, r);
    });
    return launched("fe_env_rollout_linear");
}

int fe_policy_table(fe_env *env, const double *weights, double *table, double *wsum, void *stream) {
    if (!env || !weights || !table || !wsum) return fail(FE_ERR_ARG, "fe_policy_table: null argument");
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    const Params &p = env->p;
    const int64_t entries = p.D * p.L * p.A;
    int64_t blocks = (entries * 64 + kBlock - 1) / kBlock;
    if (blocks > 256 * 16) blocks = 256 * 16;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(fe_policy_table_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, p, weights,
                       table, wsum);
    return launched("fe_policy_table");
}

int fe_env_rollout_table(fe_env *env, const double *table, const double *wsum, double bias, int32_t K,
                         int64_t *obs_src, double *obs_pos, float *actions_out, double *rewards_out,
                         int32_t *dones_out, void *stream) {
    if (!env || !table || !wsum || !obs_src || !obs_pos || !rewards_out || !dones_out || K < 1)
        return fail(FE_ERR_ARG, "fe_env_rollout_table: bad argument");
    if (int rc = require_bound(env, "fe_env_rollout_table")) return rc;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    Params p = env->p;
    // lane-private loop (no LDS traffic at one asset): full workgroups of sleeves
    const int64_t grid = rollout_geometry(env, p, kBlock, /*replace=*/false);
    TableRolloutArgs r;
    r.table = table; r.wsum = wsum; r.bias = bias; r.K = K; r.obs_src = obs_src; r.obs_pos = obs_pos;
    r.actions_out = actions_out; r.rew_out = rewards_out; r.done_out = dones_out;
    const size_t lds = table_rollout_lds_bytes(p.EB, p.A);
    with_bool(p.A == 1, [&](auto S) {
        hipLaunchKernelGGL(fe_rollout_table_kernel<decltype(S)::value>, dim3((unsigned)grid), dim3(kBlock), lds,
                           (hipStream_t)stream, p, r);
    });
    return launched("fe_env_rollout_table");
}

// The hidden sizes the MLP kernels and the register-resident LSTM kernels are instantiated for (with_nt).
static bool resident_h_ok(int32_t H) { return H == 32 || H == 64 || H == 128; }

// What every MLP entry refuses about the network's shape, in `who`'s name.
static int mlp_shape_checked(int32_t H, int32_t activation, const char *who) {
    if (!resident_h_ok(H)) return fail(FE_ERR_ARG, "%s: H must be 32, 64 or 128 (got %d)", who, (int)H);
    if (activation < 0 || activation > 2) return fail(FE_ERR_ARG, "%s: activation must be 0 (ELU), 1 (ReLU) or 2 (tanh)", who);
    return FE_OK;
}

// The MLP rollouts' default tile: 128 (env, asset) pairs per workgroup, an env's sleeves kept together.
static int64_t mlp_tile_envs(const Params &p) { return 128 / p.A > 1 ? 128 / p.A : 1; }

int fe_env_rollout_mlp(fe_env *env, const float *logret_f32, const float *w1t, const float *wpos, const float *b1,
                       const float *w2, float b2, int32_t H, int32_t activation, int32_t K, int64_t *obs_src,
                       double *obs_pos, float *actions_out, double *rewards_out, int32_t *dones_out, void *stream) {
    if (!env || !logret_f32 || !w1t || !wpos || !b1 || !w2 || !obs_src || !obs_pos || !rewards_out || !dones_out || K < 1)
        return fail(FE_ERR_ARG, "fe_env_rollout_mlp: bad argument");
    if (int rc = mlp_shape_checked(H, activation, "fe_env_rollout_mlp")) return rc;
    if (int rc = require_bound(env, "fe_env_rollout_mlp")) return rc;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    Params p = env->p;
    MlpArgs r;
    r.lr32 = logret_f32; r.w1t = w1t; r.wpos = wpos; r.b1 = b1; r.w2 = w2; r.b2 = b2; r.H = H; r.act = activation; r.K = K;
    r.obs_src = obs_src; r.obs_pos = obs_pos; r.actions_out = actions_out; r.rew_out = rewards_out; r.done_out = dones_out;
    // 128 pairs per workgroup = four 32-pair MFMA column blocks, one per wavefront, two workgroups per CU.
    // (A 512-thread form running policy and accounting of two sub-tiles in antiphase was tried and dropped: on
    // gfx950 the f32-input MFMA executes on the vector ALUs -- SQ_VALU_MFMA_COEXEC_CYCLES = 0 -- so there is
    // nothing for the accounting to hide behind; profiles/r02_microbench/mlp_prof.txt.)
    const int64_t grid = rollout_geometry(env, p, mlp_tile_envs(p), /*replace=*/true);
    const size_t lds = mlp_lds_bytes(p.EB, p.A, p.W, H);
    const void *kern = with_nt(p.A == 1, H, [](auto S, auto NT) { return (const void *)fe_rollout_mlp_kernel<decltype(S)::value, decltype(NT)::value>; });
    if (lds > kMaxLds)
        return fail(FE_ERR_ARG, "fe_env_rollout_mlp: W1 (%d x %d) does not fit the 160 KiB LDS (%zu bytes needed)", (int)H, 4 * p.W, lds);
    return launch_big_lds(env->device, kern, grid, lds, p, r, stream, "fe_env_rollout_mlp");
}

// ---- include/finenvs_amd_mlp_head.h and include/finenvs_amd_mlp2_head.h: the MLP heads trained on descriptors ----
// Either head's weights as the shared code sees them: the first layer, the second hidden layer if there is one, the output
// layer (fe_mlp_weights' w2 / b2, fe_mlp2_weights' w3 / b3).  `given`: the caller's struct and every pointer in it.
struct MlpHeadView {
    const float *w1t, *wpos, *b1;
    const float *w2h, *b2h;  // (H, H), (H): the second hidden layer; null in the one-layer head
    const float *wout, *bout;
    bool deep, given;
};

static MlpHeadView mlp_view(const fe_mlp_weights *w) {
    if (!w) return {};
    return {w->w1t, w->wpos, w->b1, nullptr, nullptr, w->w2, w->b2, false, w->w1t && w->wpos && w->b1 && w->w2 && w->b2};
}

static MlpHeadView mlp_view(const fe_mlp2_weights *w) {
    if (!w) return {};
    return {w->w1t, w->wpos, w->b1, w->w2, w->b2, w->w3, w->b3, true,
            w->w1t && w->wpos && w->b1 && w->w2 && w->b2 && w->w3 && w->b3};
}

// The checks every entry shares; `who` names it.
static int mlp_head_checked(const fe_env *env, const float *logret_f32, const MlpHeadView &w, int32_t H, int32_t activation,
                            int32_t out_activation, const char *who) {
    if (!env || !logret_f32 || !w.given) return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (int rc = mlp_shape_checked(H, activation, who)) return rc;
    if (out_activation < 0 || out_activation > 2)
        return fail(FE_ERR_ARG, "%s: out_activation must be 0 (tanh), 1 (clamp) or 2 (none)", who);
    return FE_OK;
}

// One rule for acting, values and gradients, whichever kernel runs: the weight image (W1^T, and the padded W2 of the
// deeper head) fits the LDS next to the rollout's tile of `eb` envs.
static size_t mlp_head_lds_bytes(const MlpHeadView &w, int64_t eb, const Params &p, int32_t H) {
    return w.deep ? mlp2_lds_bytes((int)eb, p.A, p.W, H) : mlp_lds_bytes((int)eb, p.A, p.W, H);
}

static int mlp_head_fits(const fe_env *env, const MlpHeadView &w, int32_t H, const char *who) {
    const Params &p = env->p;
    const size_t lds = mlp_head_lds_bytes(w, mlp_tile_envs(p), p, H);
    if (lds <= kMaxLds) return FE_OK;
    if (w.deep)
        return fail(FE_ERR_ARG, "%s: W1 (%d x %d) and W2 (%d x %d) do not fit the 160 KiB LDS: the window does not fit (%zu bytes "
                    "needed)", who, (int)H, 4 * p.W, (int)H, (int)H, lds);
    return fail(FE_ERR_ARG, "%s: W1 (%d x %d) does not fit the 160 KiB LDS (%zu bytes needed)", who, (int)H, 4 * p.W, lds);
}

// LDS of the kernels that hold only the weight image (forward, backward)
static size_t mlp_head_image_bytes(const MlpHeadView &w, int W, int32_t H) {
    return w.deep ? mlp2_weight_lds_bytes(W, H) : mlp_head_weight_lds_bytes(W, H);
}

// The argument block of either head's rollout and forward kernels: a one-layer kernel takes the leading MlpHeadArgs.
static Mlp2HeadArgs mlp_head_args(const float *logret_f32, const MlpHeadView &w, int32_t H, int32_t activation,
                                  int32_t out_activation) {
    Mlp2HeadArgs r;
    memset(&r, 0, sizeof(r));
    r.h.lr32 = logret_f32; r.h.w1t = w.w1t; r.h.wpos = w.wpos; r.h.b1 = w.b1; r.h.w2 = w.wout; r.h.b2 = w.bout;
    r.h.H = H; r.h.act = activation; r.h.out_act = out_activation; r.h.K = 1;
    r.w2h = w.w2h; r.b2h = w.b2h;
    return r;
}

// Either head's kernels at (A == 1, H): the sampled rollout, the forward, the backward's first launch and the layer-1
// weight gradient both backward passes end with.  Named here and in this order on purpose: the device code object lists
// its template instantiations as the host code first names them, and that object stays byte for byte what it was.
struct MlpHeadKernels { const void *sampled, *forward, *grad, *wgrad; };

static MlpHeadKernels mlp_head_kernels(bool deep, bool single, int32_t H) {
    MlpHeadKernels k;
    if (!deep) {
        k.sampled = with_nt(single, H, [](auto S, auto NT) { return (const void *)fe_rollout_mlp_sampled_kernel<decltype(S)::value, decltype(NT)::value>; });
        k.forward = with_nt(single, H, [](auto S, auto NT) { return (const void *)fe_mlp_forward_kernel<decltype(S)::value, decltype(NT)::value>; });
        k.grad = with_nt(H, [](auto NT) { return (const void *)fe_mlp_grad_kernel<decltype(NT)::value>; });
    }
    k.wgrad = with_nt(H, [](auto NT) { return (const void *)fe_mlp_wgrad_kernel<decltype(NT)::value>; });
    if (deep) {
        k.sampled = with_nt(single, H, [](auto S, auto NT) { return (const void *)fe_rollout_mlp2_sampled_kernel<decltype(S)::value, decltype(NT)::value>; });
        k.forward = with_nt(single, H, [](auto S, auto NT) { return (const void *)fe_mlp2_forward_kernel<decltype(S)::value, decltype(NT)::value>; });
        k.grad = with_nt(H, [](auto NT) { return (const void *)fe_mlp2_grad_kernel<decltype(NT)::value>; });
    }
    return k;
}

int fe_mlp_pack(const float *weight1, int32_t H, int32_t W, float *w1t, float *wpos, void *stream) {
    if (!weight1 || !w1t || !wpos) return fail(FE_ERR_ARG, "fe_mlp_pack: bad argument");
    if (!resident_h_ok(H)) return fail(FE_ERR_ARG, "fe_mlp_pack: H must be 32, 64 or 128 (got %d)", (int)H);
    if (W < 1) return fail(FE_ERR_ARG, "fe_mlp_pack: W must be >= 1 (got %d)", (int)W);
    DeviceGuard guard(device_of(weight1));
    if (int rc = guard.status()) return rc;
    hipLaunchKernelGGL(fe_mlp_pack_kernel, dim3(grid_for((int64_t)H * 4 * W + H)), dim3(kBlock), 0, (hipStream_t)stream, weight1,
                       (int)H, (int)W, w1t, wpos);
    return launched("fe_mlp_pack");
}

// fe_env_rollout_mlp_sampled and fe_env_rollout_mlp2_sampled
static int rollout_mlp_sampled_impl(fe_env *env, const float *logret_f32, const MlpHeadView &w, int32_t H, int32_t activation,
                                    int32_t out_activation, int32_t K, int64_t *obs_src, double *obs_pos, const float *noise,
                                    float std, float *actions_out, float *means_out, double *rewards_out, int32_t *dones_out,
                                    int64_t *states_src_out, double *states_pos_out, void *stream, const char *who) {
    if ((states_src_out == nullptr) != (states_pos_out == nullptr))
        return fail(FE_ERR_ARG, "%s: states_src_out and states_pos_out go together", who);
    if (noise && !(std >= 0.0f)) return fail(FE_ERR_ARG, "%s: std must be >= 0 when noise is given", who);
    if (!obs_src || !obs_pos || !rewards_out || !dones_out || K < 1) return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (int rc = mlp_head_checked(env, logret_f32, w, H, activation, out_activation, who)) return rc;
    if (int rc = require_bound(env, who)) return rc;
    if (int rc = mlp_head_fits(env, w, H, who)) return rc;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    Params p = env->p;
    Mlp2HeadArgs r = mlp_head_args(logret_f32, w, H, activation, out_activation);
    r.h.K = K; r.h.obs_src = obs_src; r.h.obs_pos = obs_pos;
    r.h.noise = noise; r.h.std = std; r.h.actions_out = actions_out; r.h.means_out = means_out; r.h.rew_out = rewards_out;
    r.h.done_out = dones_out; r.h.traj_src = states_src_out; r.h.traj_pos = states_pos_out;
    // the geometry of fe_env_rollout_mlp: 128 pairs per workgroup, one 32-pair column block per wavefront
    const int64_t grid = rollout_geometry(env, p, mlp_tile_envs(p), /*replace=*/true);
    const size_t lds = mlp_head_lds_bytes(w, p.EB, p, H);
    const void *kern = mlp_head_kernels(w.deep, p.A == 1, H).sampled;
    if (lds > kMaxLds) {  // (a tile override larger than the default)
        if (w.deep) return fail(FE_ERR_ARG, "%s: the weight image does not fit the 160 KiB LDS at this tile (%zu bytes needed)", who, lds);
        return fail(FE_ERR_ARG, "%s: W1 (%d x %d) does not fit the 160 KiB LDS (%zu bytes needed)", who, (int)H, 4 * p.W, lds);
    }
    return launch_big_lds(env->device, kern, grid, lds, p, r, stream, who);
}

int fe_env_rollout_mlp_sampled(fe_env *env, const float *logret_f32, const fe_mlp_weights *weights, int32_t H,
                               int32_t activation, int32_t out_activation, int32_t K, int64_t *obs_src, double *obs_pos,
                               const float *noise, float std, float *actions_out, float *means_out, double *rewards_out,
                               int32_t *dones_out, int64_t *states_src_out, double *states_pos_out, void *stream) {
    return rollout_mlp_sampled_impl(env, logret_f32, mlp_view(weights), H, activation, out_activation, K, obs_src, obs_pos, noise,
                                    std, actions_out, means_out, rewards_out, dones_out, states_src_out, states_pos_out, stream,
                                    "fe_env_rollout_mlp_sampled");
}

int fe_env_rollout_mlp2_sampled(fe_env *env, const float *logret_f32, const fe_mlp2_weights *weights, int32_t H,
                                int32_t activation, int32_t out_activation, int32_t K, int64_t *obs_src, double *obs_pos,
                                const float *noise, float std, float *actions_out, float *means_out, double *rewards_out,
                                int32_t *dones_out, int64_t *states_src_out, double *states_pos_out, void *stream) {
    return rollout_mlp_sampled_impl(env, logret_f32, mlp_view(weights), H, activation, out_activation, K, obs_src, obs_pos, noise,
                                    std, actions_out, means_out, rewards_out, dones_out, states_src_out, states_pos_out, stream,
                                    "fe_env_rollout_mlp2_sampled");
}

// fe_mlp_forward and fe_mlp2_forward
static int mlp_forward_impl(fe_env *env, const float *logret_f32, const MlpHeadView &w, int32_t H, int32_t activation,
                            int32_t out_activation, const int64_t *obs_src, const double *obs_pos, int64_t count, float *out,
                            void *stream, const char *who) {
    if (!obs_src || !obs_pos || !out || count < 0) return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (int rc = mlp_head_checked(env, logret_f32, w, H, activation, out_activation, who)) return rc;
    if (int rc = mlp_head_fits(env, w, H, who)) return rc;
    if (count == 0) return FE_OK;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    Params p = env->p;
    Mlp2HeadArgs r = mlp_head_args(logret_f32, w, H, activation, out_activation);
    r.h.obs_src = const_cast<int64_t *>(obs_src); r.h.obs_pos = const_cast<double *>(obs_pos);  // read only in this kernel
    r.h.actions_out = out; r.h.count = count;
    const int64_t blocks = (count * p.A + 31) / 32;
    const int64_t grid = capped_grid((blocks + kBlock / 64 - 1) / (kBlock / 64));
    const void *kern = mlp_head_kernels(w.deep, p.A == 1, H).forward;
    return launch_big_lds(env->device, kern, grid, mlp_head_image_bytes(w, p.W, H), p, r, stream, who);
}

int fe_mlp_forward(fe_env *env, const float *logret_f32, const fe_mlp_weights *weights, int32_t H, int32_t activation,
                   int32_t out_activation, const int64_t *obs_src, const double *obs_pos, int64_t count, float *out,
                   void *stream) {
    return mlp_forward_impl(env, logret_f32, mlp_view(weights), H, activation, out_activation, obs_src, obs_pos, count, out, stream,
                            "fe_mlp_forward");
}

int fe_mlp2_forward(fe_env *env, const float *logret_f32, const fe_mlp2_weights *weights, int32_t H, int32_t activation,
                    int32_t out_activation, const int64_t *obs_src, const double *obs_pos, int64_t count, float *out,
                    void *stream) {
    return mlp_forward_impl(env, logret_f32, mlp_view(weights), H, activation, out_activation, obs_src, obs_pos, count, out, stream,
                            "fe_mlp2_forward");
}

// The backward passes' workspace, in floats from its start, for either depth (a1, dz2 and part2 are the deeper head's):
// [dpre = dz1 (32 blocks, H)][a1][dz2][layer-1 partials (splits, H, FP)][[dW2 | d b2] partials (splits, H, H + 32)]
// [output-layer partials (waves, H + 4)].  The exported sizes and the carve-up both read it.
struct MlpGradLayout {
    int64_t blocks, splits, groups;
    int32_t FP;
    int64_t a1, dz2, part, part2, wpart, total;
};

static MlpGradLayout mlp_grad_layout(bool deep, int32_t H, int32_t W, int64_t count) {
    MlpGradLayout l;
    l.blocks = (count + 31) / 32;
    l.splits = (count + kMlpGradChunk - 1) / kMlpGradChunk;
    l.groups = mlp_grad_groups(l.blocks);
    l.FP = mlp_grad_fp(W);
    const int64_t rows = 32 * l.blocks * H;
    l.a1 = rows;
    l.dz2 = 2 * rows;
    l.part = deep ? 3 * rows : rows;
    l.part2 = l.part + l.splits * H * l.FP;
    l.wpart = l.part2 + (deep ? l.splits * H * (H + 32) : 0);
    l.total = l.wpart + 4 * l.groups * (H + 4);
    return l;
}

static int64_t mlp_grad_workspace_floats(bool deep, int32_t H, int32_t W, int64_t count) {
    if (!resident_h_ok(H) || W < 1 || count < 0) return -1;
    return count == 0 ? 0 : mlp_grad_layout(deep, H, W, count).total;
}

int64_t fe_mlp_grad_workspace_floats(int32_t H, int32_t W, int64_t count) { return mlp_grad_workspace_floats(false, H, W, count); }

int64_t fe_mlp2_grad_workspace_floats(int32_t H, int32_t W, int64_t count) { return mlp_grad_workspace_floats(true, H, W, count); }

// What both backward entries refuse, in this order.  `given`: the entry's own pointers and its gradient struct are there.
static int mlp_backward_checked(const fe_env *env, const float *logret_f32, const MlpHeadView &w, int32_t H, int32_t activation,
                                int32_t out_activation, bool given, const float *outputs, const char *who) {
    if (!given) return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (int rc = mlp_head_checked(env, logret_f32, w, H, activation, out_activation, who)) return rc;
    if (out_activation == 1)
        return fail(FE_ERR_ARG, "%s: out_activation must be 0 (tanh) or 2 (none); 1 (clamp) has no gradient to train on", who);
    if (out_activation == 0 && !outputs)
        return fail(FE_ERR_ARG, "%s: out_activation 0 (tanh) needs outputs, the values %s returned", who,
                    w.deep ? "fe_mlp2_forward" : "fe_mlp_forward");
    if (env->p.A != 1)
        return fail(FE_ERR_ARG, "%s: the env has %d assets; the fused head gradient runs A = 1 only (as the fused LSTM "
                    "head does)", who, (int)env->p.A);
    return mlp_head_fits(env, w, H, who);
}

// The arguments of the layer-1 and output-layer kernels; g_wout / g_bout: the output layer's gradients.
static MlpGradArgs mlp_grad_args(const float *logret_f32, const MlpHeadView &w, int32_t H, int32_t W, int32_t activation,
                                 int32_t out_activation, const int64_t *obs_src, const double *obs_pos, int64_t count,
                                 const float *outputs, const float *d_outputs, float *workspace, const MlpGradLayout &l,
                                 float *g_w1, float *g_b1, float *g_wout, float *g_bout) {
    MlpGradArgs g;
    memset(&g, 0, sizeof(g));
    g.lr32 = logret_f32; g.w1t = w.w1t; g.wpos = w.wpos; g.b1 = w.b1; g.w2 = w.wout;
    g.obs_src = obs_src; g.obs_pos = obs_pos; g.outputs = outputs; g.d_outputs = d_outputs;
    g.count = count; g.blocks = l.blocks; g.splits = l.splits; g.waves = 4 * l.groups;
    g.W = W; g.H = H; g.act = activation; g.out_act = out_activation; g.FP = l.FP;
    g.dpre = workspace; g.part = workspace + l.part; g.wpart = workspace + l.wpart;
    g.g_w1 = g_w1; g.g_b1 = g_b1; g.g_w2 = g_wout; g.g_b2 = g_bout;
    return g;
}

// The first layer's weight gradient (`kern`, its step named `wgrad_step`) and the reduction of layer 1 and the output layer.
static int mlp_backward_layer1(MlpGradArgs &g, const void *kern, const char *who, const char *wgrad_step, hipStream_t st) {
    void *args[] = {&g};
    const int64_t items = g.splits * (g.FP / 32);
    const int64_t grid = capped_grid((items + kBlock / 64 - 1) / (kBlock / 64));
    if (int rc = launched(who, wgrad_step, hipLaunchKernel(kern, dim3((unsigned)grid), dim3(kBlock), args, 0, st))) return rc;
    hipLaunchKernelGGL(fe_mlp_grad_reduce_kernel, dim3(grid_for((int64_t)g.H * (4 * g.W + 2) + g.H + 1)), dim3(kBlock), 0, st, g);
    return launched(who, "reduction");
}

int fe_mlp_backward(fe_env *env, const float *logret_f32, const fe_mlp_weights *weights, int32_t H, int32_t activation,
                    int32_t out_activation, const int64_t *obs_src, const double *obs_pos, int64_t count,
                    const float *outputs, const float *d_outputs, float *workspace, const fe_mlp_grads *grads,
                    void *stream) {
    static const char *who = "fe_mlp_backward";
    const MlpHeadView w = mlp_view(weights);
    const bool given = obs_src && obs_pos && count >= 0 && d_outputs && workspace && grads && grads->w1 && grads->b1 &&
                       grads->w2 && grads->b2;
    if (int rc = mlp_backward_checked(env, logret_f32, w, H, activation, out_activation, given, outputs, who)) return rc;
    if (count == 0) return FE_OK;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    const int W = env->p.W;
    const MlpGradLayout l = mlp_grad_layout(false, H, W, count);
    MlpGradArgs g = mlp_grad_args(logret_f32, w, H, W, activation, out_activation, obs_src, obs_pos, count, outputs, d_outputs,
                                  workspace, l, grads->w1, grads->b1, grads->w2, grads->b2);
    void *args[] = {&g};
    const hipStream_t st = (hipStream_t)stream;
    const MlpHeadKernels k = mlp_head_kernels(false, true, H);
    const size_t lds = mlp_head_image_bytes(w, W, H);
    if (int rc = prepare_big_lds(env->device, k.grad, lds, who)) return rc;
    if (int rc = launched(who, "first layer", hipLaunchKernel(k.grad, dim3((unsigned)l.groups), dim3(kBlock), args, lds, st))) return rc;
    return mlp_backward_layer1(g, k.wgrad, who, "weight gradient", st);
}

int fe_mlp2_backward(fe_env *env, const float *logret_f32, const fe_mlp2_weights *weights, int32_t H, int32_t activation,
                     int32_t out_activation, const int64_t *obs_src, const double *obs_pos, int64_t count,
                     const float *outputs, const float *d_outputs, float *workspace, const fe_mlp2_grads *grads,
                     void *stream) {
    static const char *who = "fe_mlp2_backward";
    const MlpHeadView w = mlp_view(weights);
    const bool given = obs_src && obs_pos && count >= 0 && d_outputs && workspace && grads && grads->w1 && grads->b1 &&
                       grads->w2 && grads->b2 && grads->w3 && grads->b3;
    if (int rc = mlp_backward_checked(env, logret_f32, w, H, activation, out_activation, given, outputs, who)) return rc;
    if (count == 0) return FE_OK;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    const int W = env->p.W;
    const MlpGradLayout l = mlp_grad_layout(true, H, W, count);
    Mlp2GradArgs g2;
    memset(&g2, 0, sizeof(g2));
    g2.g = mlp_grad_args(logret_f32, w, H, W, activation, out_activation, obs_src, obs_pos, count, outputs, d_outputs, workspace,
                         l, grads->w1, grads->b1, grads->w3, grads->b3);
    g2.a1 = workspace + l.a1; g2.dz2 = workspace + l.dz2; g2.part2 = workspace + l.part2;
    g2.w2h = w.w2h; g2.b2h = w.b2h; g2.g_w2h = grads->w2; g2.g_b2h = grads->b2;
    void *args2[] = {&g2};
    const hipStream_t st = (hipStream_t)stream;
    const int64_t wave_groups = capped_grid((l.blocks + kBlock / 64 - 1) / (kBlock / 64));
    // (1) both hidden layers recomputed: a1, dz2, the partials of d w3 / d b3
    const MlpHeadKernels k = mlp_head_kernels(true, true, H);
    const size_t lds1 = mlp_head_image_bytes(w, W, H);
    if (int rc = prepare_big_lds(env->device, k.grad, lds1, who)) return rc;
    if (int rc = launched(who, "hidden layers", hipLaunchKernel(k.grad, dim3((unsigned)l.groups), dim3(kBlock), args2, lds1, st))) return rc;
    // (2) dz1 = (W2^T dz2) * act'(z1)
    const void *k2 = with_nt(H, [](auto NT) { return (const void *)fe_mlp2_dgrad_kernel<decltype(NT)::value>; });
    const size_t lds2 = (size_t)H * mlp2_hp(H) * 4;
    if (int rc = prepare_big_lds(env->device, k2, lds2, who)) return rc;
    if (int rc = launched(who, "W2^T dz2", hipLaunchKernel(k2, dim3((unsigned)wave_groups), dim3(kBlock), args2, lds2, st))) return rc;
    // (3) [dW2 | d b2] partials
    const void *k3 = with_nt(H, [](auto NT) { return (const void *)fe_mlp2_wgrad2_kernel<decltype(NT)::value>; });
    const int64_t items3 = l.splits * (H / 32 + 1);
    const int64_t grid3 = capped_grid((items3 + kBlock / 64 - 1) / (kBlock / 64));
    if (int rc = launched(who, "dz2^T a1", hipLaunchKernel(k3, dim3((unsigned)grid3), dim3(kBlock), args2, 0, st))) return rc;
    // (4), (5) the first layer's weight gradient and the output layer's partials: fe_mlp_backward's kernels on dz1
    if (int rc = mlp_backward_layer1(g2.g, k.wgrad, who, "first-layer weight gradient", st)) return rc;
    // (6) the second hidden layer's reduction
    hipLaunchKernelGGL(fe_mlp2_grad_reduce_kernel, dim3(grid_for((int64_t)H * (H + 1))), dim3(kBlock), 0, st, g2);
    return launched(who, "W2 reduction");
}

// ---- the LSTM family: the one-output head, the SAC actor and the twin critics, register-resident (H = 32 / 64 / 128) and
// streamed (H = 256 / 512 / 1024).  An entry and its streamed namesake share one implementation, told which it serves. ----
// The one-output head's weights as the shared code sees them (after MlpHeadView).  The output bias travels by value or,
// bout_p non-null, is read on the device (the *_p entries of include/finenvs_amd_optim.h); a backward pass needs neither.
struct LstmHeadView { const float *whh, *wx, *wout; float bout; const float *bout_p; };
static bool lstm_view_given(const LstmHeadView &w) { return w.whh && w.wx && w.wout; }

// The SAC actor's weights likewise: the two head biases by value or, non-null, on the device (the *_p and the streamed
// entries, which refuse a null one before they fill this).
struct SacActorView { const float *whh, *wx, *wl, *bl, *wmu, *wstd; float bmu, bstd; const float *bmu_p, *bstd_p; };
static bool sac_view_given(const SacActorView &w) { return w.whh && w.wx && w.wl && w.bl && w.wmu && w.wstd; }

// What an entry refuses when its kernel's workgroup does not fit the LDS at this H.
static int lds_fits(size_t lds, int32_t H, const char *who) {
    if (lds <= kMaxLds) return FE_OK;
    return fail(FE_ERR_ARG, "%s: H = %d needs %zu bytes of LDS per workgroup, the device has %zu", who, (int)H, lds, kMaxLds);
}

// Tile geometry of the fused LSTM kernels (LSTM and SAC heads) for `count` envs (rollout) or descriptors (forward): sets
// p.N, p.EB, p.num_tiles; returns the workgroup tile's (env, asset) pairs SP, or 0 after fail() when an env's sleeves do
// not fit one tile.
static int lstm_geometry(const fe_env *env, Params &p, int64_t count, int32_t H, bool big, const char *who) {
    p.N = count;
    // SP (env, asset) pairs per workgroup: 1 (H >= 256), 2 (H = 128) or 4 column tiles of 32; an env's sleeves stay together
    const int SP = big ? 32 : (H == 128 ? LstmGeom<4>::SP : LstmGeom<2>::SP);
    if (p.A > SP) {
        fail(FE_ERR_ARG, "%s: %d assets per env exceed the %d pairs of a workgroup tile (H = %d)", who, (int)p.A, SP, (int)H);
        return 0;
    }
    int64_t eb = SP / p.A;
    // few envs: a tile lives on one CU for a whole step, so spread them over the CUs -- halve the tile (down to one
    // 32-pair column tile) while that fills otherwise idle CUs; a wavefront then runs fewer column tiles per time step
    const int64_t min_eb = 32 / p.A > 1 ? 32 / p.A : 1;
    while (!big && eb > min_eb && (p.N + eb - 1) / eb < env->cus) eb = eb / 2 > min_eb ? eb / 2 : min_eb;
    if (env->rollout_tile_override > 0 && env->rollout_tile_override < eb) eb = env->rollout_tile_override;
    p.EB = (int)eb;
    p.num_tiles = (p.N + eb - 1) / eb;
    return SP;
}

// One pass of resident kLstmBlock-thread workgroups, each looping over its tiles; `r` is the kernel's argument block after
// the Params.  `what` names the kernel in errors.
static int launch_resident(const fe_env *env, const void *kern, size_t lds, Params &p, void *r, const char *what, void *stream) {
    int per_cu = 0;
    hipError_t he = prepare_kernel(env->device, kern, kLstmBlock, lds, &per_cu);
    if (he != hipSuccess) {
        char msg[64];
        snprintf(msg, sizeof(msg), "%s: hipFuncSetAttribute / occupancy query", what);
        return hip_fail(he, msg);
    }
    const int64_t resident = (int64_t)env->cus * per_cu;
    const int64_t grid = p.num_tiles < resident ? p.num_tiles : resident;
    void *args[] = {&p, r};
    return launched(what, hipLaunchKernel(kern, dim3((unsigned)grid), dim3(kLstmBlock), args, lds, (hipStream_t)stream));
}

// The fused backward passes (fe_bptt_tile.h): 32-pair tiles, and the workgroups that own partials and a stash in the
// workspace -- one per tile up to `cap`, the kernel's resident count on an MI355X.
struct GradTiles { int64_t tiles, max_groups; };
static GradTiles grad_tiles(int64_t count, int64_t cap) {
    const int64_t tiles = (count + 31) / 32;
    return {tiles, tiles < cap ? tiles : cap};
}

// Their main pass: resident kBpttBlock-thread workgroups, at most max_groups per grid row (`rows` rows share the
// device), each looping over its tiles.  `g` is the kernel's one argument, *groups its field for the row length.
// `what` names the kernel in a preparation error, `step` the launch.
static int launch_grad(const fe_env *env, const void *kern, size_t lds, int64_t max_groups, int rows, void *g,
                       int64_t *groups, const char *what, const char *step, void *stream) {
    int per_cu = 0;
    const hipError_t he = prepare_kernel(env->device, kern, kBpttBlock, lds, &per_cu);
    if (he != hipSuccess) return hip_fail(he, what);
    int64_t resident = (int64_t)env->cus * per_cu / rows;
    if (resident < 1) resident = 1;
    *groups = max_groups < resident ? max_groups : resident;
    void *args[] = {g};
    return launched(step, hipLaunchKernel(kern, dim3((unsigned)*groups, rows), dim3(kBpttBlock), args, lds, (hipStream_t)stream));
}

// Shared by fe_env_rollout_lstm and fe_lstm_forward: geometry, kernel choice, launch.  `count` = envs (rollout) or
// descriptors (forward).
static int launch_lstm(fe_env *env, LstmArgs &r, int64_t count, const char *who, void *stream) {
    const int32_t H = r.H;
    const bool big = lstm_sgrad_hidden_ok(H);  // weights streamed from L2 (fragment-major whh)
    if (!resident_h_ok(H) && !big)
        return fail(FE_ERR_ARG, "%s: H must be 32, 64, 128, 256, 512 or 1024 (got %d)", who, (int)H);
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    Params p = env->p;
    const int SP = lstm_geometry(env, p, count, H, big, who);
    if (SP == 0) return FE_ERR_ARG;
    const size_t lds = big ? lstm_big_lds_bytes(p.EB, p.A, H) : lstm_lds_bytes(p.EB, p.A, H, SP);
    const void *kern = with_bool(p.A == 1, [H, big](auto S) {  // (with_bool outermost: the instantiations keep their order)
        if (!big) return with_nt(H, [](auto NT) { return (const void *)fe_rollout_lstm_kernel<decltype(S)::value, decltype(NT)::value>; });
        return with_nt<64, 4>(H, [](auto NT) { return (const void *)fe_rollout_lstm_big_kernel<decltype(S)::value, decltype(NT)::value>; });
    });
    return launch_resident(env, kern, lds, p, &r, "LSTM kernel", stream);
}

// Shared by fe_env_rollout_sac and fe_sac_forward.  The forward form has no evaluation env: every descriptor with noise
// samples.
static int launch_sac(fe_env *env, SacArgs &s, int64_t count, const char *who, void *stream) {
    const int32_t H = s.l.H;
    if (!resident_h_ok(H))
        return fail(FE_ERR_ARG, "%s: H must be 32, 64 or 128 (got %d): the SAC head has no streamed or split kernel", who, (int)H);
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    Params p = env->p;
    if (s.l.forward_only) p.eval_env = -1;
    const int SP = lstm_geometry(env, p, count, H, false, who);
    if (SP == 0) return FE_ERR_ARG;
    const size_t lds = sac_lds_bytes(p.EB, p.A, H, SP);
    const void *kern = with_nt(p.A == 1, H, [](auto S, auto NT) { return (const void *)fe_rollout_sac_kernel<decltype(S)::value, decltype(NT)::value>; });
    return launch_resident(env, kern, lds, p, &s, "SAC kernel", stream);
}

// The *_impl functions serve an entry that takes its output bias by value and its sibling of
// include/finenvs_amd_optim.h that reads it through a device pointer (bout_p etc. non-null).
// The head's part of a kernel's LstmArgs.
static void lstm_args(LstmArgs &r, const float *logret_f32, const LstmHeadView &w, int32_t H, int32_t out_activation) {
    r.lr32 = logret_f32; r.whh = w.whh; r.wx = w.wx; r.wout = w.wout; r.bout = w.bout; r.bout_p = w.bout_p; r.H = H;
    r.out_act = out_activation;
}

static int rollout_lstm_impl(fe_env *env, const float *logret_f32, const LstmHeadView &w, int32_t H, int32_t out_activation,
                             int32_t K, int64_t *obs_src, double *obs_pos, const float *noise, float std, float *actions_out,
                             float *means_out, double *rewards_out, int32_t *dones_out, int64_t *states_src_out,
                             double *states_pos_out, void *stream) {
    if ((states_src_out == nullptr) != (states_pos_out == nullptr))
        return fail(FE_ERR_ARG, "fe_env_rollout_lstm: states_src_out and states_pos_out go together");
    if (noise && !(std >= 0.0f)) return fail(FE_ERR_ARG, "fe_env_rollout_lstm: std must be >= 0 when noise is given");
    if (!env || !logret_f32 || !lstm_view_given(w) || !obs_src || !obs_pos || !rewards_out || !dones_out || K < 1)
        return fail(FE_ERR_ARG, "fe_env_rollout_lstm: bad argument");
    if (out_activation < 0 || out_activation > 1) return fail(FE_ERR_ARG, "fe_env_rollout_lstm: out_activation must be 0 (tanh) or 1 (clamp)");
    if (int rc = require_bound(env, "fe_env_rollout_lstm")) return rc;
    LstmArgs r;
    lstm_args(r, logret_f32, w, H, out_activation);
    r.K = K;
    r.obs_src = obs_src; r.obs_pos = obs_pos; r.actions_out = actions_out; r.rew_out = rewards_out; r.done_out = dones_out;
    r.noise = noise; r.std = std; r.means_out = means_out; r.traj_src = states_src_out; r.traj_pos = states_pos_out;
    r.forward_only = 0;
    return launch_lstm(env, r, env->cfg.N, "fe_env_rollout_lstm", stream);
}

int fe_env_rollout_lstm(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wout,
                        float bout, int32_t H, int32_t out_activation, int32_t K, int64_t *obs_src, double *obs_pos,
                        const float *noise, float std, float *actions_out, float *means_out, double *rewards_out,
                        int32_t *dones_out, int64_t *states_src_out, double *states_pos_out, void *stream) {
    return rollout_lstm_impl(env, logret_f32, {whh, wx, wout, bout, nullptr}, H, out_activation, K, obs_src, obs_pos, noise, std,
                             actions_out, means_out, rewards_out, dones_out, states_src_out, states_pos_out, stream);
}

int64_t fe_lstm_split_workspace_floats(int32_t H, int64_t pairs) {
    if (H < 8 || pairs < 1) return 0;
    return 3 * ((pairs + 31) / 32) * (int64_t)H * 32;  // h (two buffers) + c, fragment-major: [column tile][H/8][64][4]
}

static int rollout_lstm_split_impl(fe_env *env, const float *logret_f32, const LstmHeadView &w, int32_t H,
                                   int32_t out_activation, int32_t K, int64_t *obs_src, double *obs_pos, const float *noise,
                                   float std, float *actions_out, float *means_out, double *rewards_out, int32_t *dones_out,
                                   int64_t *states_src_out, double *states_pos_out, float *workspace, void *stream) {
    if ((states_src_out == nullptr) != (states_pos_out == nullptr))
        return fail(FE_ERR_ARG, "fe_env_rollout_lstm_split: states_src_out and states_pos_out go together");
    if (noise && !(std >= 0.0f)) return fail(FE_ERR_ARG, "fe_env_rollout_lstm_split: std must be >= 0 when noise is given");
    if (!env || !logret_f32 || !lstm_view_given(w) || !obs_src || !obs_pos || !rewards_out || !dones_out || !workspace || K < 1)
        return fail(FE_ERR_ARG, "fe_env_rollout_lstm_split: bad argument");
    if (!lstm_sgrad_hidden_ok(H))
        return fail(FE_ERR_ARG, "fe_env_rollout_lstm_split: H must be 256, 512 or 1024 (got %d)", (int)H);
    if (out_activation < 0 || out_activation > 1)
        return fail(FE_ERR_ARG, "fe_env_rollout_lstm_split: out_activation must be 0 (tanh) or 1 (clamp)");
    if (int rc = require_bound(env, "fe_env_rollout_lstm_split")) return rc;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    Params p = env->p;
    const int64_t NA = p.N * p.A, CT = (NA + 31) / 32;
    // the accounting launch: few sleeves per workgroup, so that a handful of envs still spreads over the CUs
    // (and their h_W rows, 4 H bytes per pair, are staged in LDS)
    const int64_t fgrid = rollout_geometry(env, p, 16 / p.A > 1 ? 16 / p.A : 1, /*replace=*/false);
    const size_t lds = ((table_rollout_lds_bytes(p.EB, p.A) + 15) & ~(size_t)15) + (size_t)p.EB * p.A * H * 4;
    if (lds > kMaxLds)
        return fail(FE_ERR_ARG, "fe_env_rollout_lstm_split: %d sleeves per env x H = %d do not fit the LDS of the accounting launch", (int)p.A, (int)H);
    const bool single = p.A == 1;
    const void *fk = with_bool(single, [](auto S) { return (const void *)fe_lstm_split_finish_kernel<decltype(S)::value>; });
    if (int rc = prepare_big_lds(env->device, fk, lds, "fe_env_rollout_lstm_split")) return rc;
    LstmSplitArgs s;
    lstm_args(s.a, logret_f32, w, H, out_activation);
    s.a.K = 1; s.a.obs_src = obs_src; s.a.obs_pos = obs_pos; s.a.std = std; s.a.traj_src = states_src_out; s.a.traj_pos = states_pos_out;
    s.a.forward_only = 0;
    s.hbuf = workspace; s.cbuf = workspace + 2 * CT * (int64_t)H * 32; s.pairs = NA;
    const dim3 ggrid((unsigned)(H / 8), (unsigned)((CT + kBlock / 64 - 1) / (kBlock / 64)));
    const size_t glds = (size_t)(H / 8) * 64 * 16;  // one gate-row tile of weights: H / 8 KiB (128 KiB at H = 1024)
    const void *gk = with_bool(single, [](auto S) { return (const void *)fe_lstm_split_gates_kernel<decltype(S)::value>; });
    if (int rc = prepare_big_lds(env->device, gk, glds, "fe_env_rollout_lstm_split")) return rc;
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < K; ++k) {
        s.k = k;
        s.a.noise = noise ? noise + (int64_t)k * NA : nullptr;
        s.a.actions_out = actions_out ? actions_out + (int64_t)k * NA : nullptr;
        s.a.means_out = means_out ? means_out + (int64_t)k * NA : nullptr;
        s.a.rew_out = rewards_out + (int64_t)k * p.N;
        s.a.done_out = dones_out + (int64_t)k * p.N;
        for (int t = 0; t < p.W; ++t) {
            s.t = t;
            with_bool(single, [&](auto S) {
                hipLaunchKernelGGL(fe_lstm_split_gates_kernel<decltype(S)::value>, ggrid, dim3(kBlock), glds, st, p, s);
            });
            // a launch that fails (bad geometry, LDS) fails the first time: stop before queueing W * K launches on
            // half-written h / c state
            if (k == 0 && t == 0) {
                if (int rc = launched("fe_env_rollout_lstm_split: gates")) return rc;
            }
        }
        with_bool(single, [&](auto S) {
            hipLaunchKernelGGL(fe_lstm_split_finish_kernel<decltype(S)::value>, dim3((unsigned)fgrid), dim3(kBlock), lds, st, p, s);
        });
        if (k == 0) {
            if (int rc = launched("fe_env_rollout_lstm_split: accounting")) return rc;
        }
    }
    return launched("fe_env_rollout_lstm_split");
}

int fe_env_rollout_lstm_split(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wout,
                              float bout, int32_t H, int32_t out_activation, int32_t K, int64_t *obs_src, double *obs_pos,
                              const float *noise, float std, float *actions_out, float *means_out, double *rewards_out,
                              int32_t *dones_out, int64_t *states_src_out, double *states_pos_out, float *workspace,
                              void *stream) {
    return rollout_lstm_split_impl(env, logret_f32, {whh, wx, wout, bout, nullptr}, H, out_activation, K, obs_src, obs_pos,
                                   noise, std, actions_out, means_out, rewards_out, dones_out, states_src_out,
                                   states_pos_out, workspace, stream);
}

static int lstm_forward_impl(fe_env *env, const float *logret_f32, const LstmHeadView &w, int32_t H, int32_t out_activation,
                             const int64_t *obs_src, const double *obs_pos, int64_t count, float *out, void *stream) {
    if (!env || !logret_f32 || !lstm_view_given(w) || !obs_src || !obs_pos || !out || count < 0)
        return fail(FE_ERR_ARG, "fe_lstm_forward: bad argument");
    if (out_activation < 0 || out_activation > 2)
        return fail(FE_ERR_ARG, "fe_lstm_forward: out_activation must be 0 (tanh), 1 (clamp) or 2 (none)");
    if (count == 0) return FE_OK;
    LstmArgs r;
    lstm_args(r, logret_f32, w, H, out_activation);
    r.K = 1;
    r.obs_src = const_cast<int64_t *>(obs_src); r.obs_pos = const_cast<double *>(obs_pos);  // read only in this mode
    r.actions_out = out; r.rew_out = nullptr; r.done_out = nullptr;
    r.noise = nullptr; r.std = 0.0f; r.means_out = nullptr; r.traj_src = nullptr; r.traj_pos = nullptr;
    r.forward_only = 1;
    return launch_lstm(env, r, count, "fe_lstm_forward", stream);
}

int fe_lstm_forward(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wout, float bout,
                    int32_t H, int32_t out_activation, const int64_t *obs_src, const double *obs_pos, int64_t count,
                    float *out, void *stream) {
    return lstm_forward_impl(env, logret_f32, {whh, wx, wout, bout, nullptr}, H, out_activation, obs_src, obs_pos, count, out,
                             stream);
}

int fe_lstm_activations(const float *x, float *sigmoid_out, float *tanh_out, int64_t n, void *stream) {
    if (!x || !sigmoid_out || !tanh_out || n < 0) return fail(FE_ERR_ARG, "fe_lstm_activations: bad argument");
    if (n == 0) return FE_OK;
    DeviceGuard guard(device_of(x));
    if (int rc = guard.status()) return rc;
    int64_t grid = (n + kBlock - 1) / kBlock;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(fe_lstm_activations_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, x, sigmoid_out, tanh_out, n);
    return launched("fe_lstm_activations");
}

int fe_env_set_day(fe_env *env, int64_t env_index, int64_t day, void *stream) {
    if (!env || !env->bound) return fail(FE_ERR_STATE, "fe_env_set_day: env not bound");
    if (env_index < 0 || env_index >= env->cfg.N || day < 0 || day >= env->cfg.D)
        return fail(FE_ERR_ARG, "fe_env_set_day: env %lld / day %lld out of range", (long long)env_index, (long long)day);
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    // a one-lane launch with the day as a kernel argument: stream-ordered behind the step that finished the episode and
    // ahead of the next one, WITHOUT a host synchronisation (round 3 copied a stack variable and had to wait for it)
    hipLaunchKernelGGL(fe_set_day_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, env->p.env_idx, env_index, day);
    return launched("fe_env_set_day");
}

int fe_env_launch_info(const fe_env *env, int32_t *grid, int32_t *block, int32_t *tile_envs, int32_t *lds) {
    if (!env) return fail(FE_ERR_ARG, "fe_env_launch_info: null env");
    if (grid) *grid = env->grid;
    if (block) *block = kBlock;
    if (tile_envs) *tile_envs = env->p.EB;
    // the kernel the NEXT step dispatches to: once the env has been stepped through fe_env_step_promoted, that one
    if (lds) *lds = (int32_t)(env->promoted_used ? env->lds_promoted : env->lds);
    return FE_OK;
}

int fe_env_set_launch(fe_env *env, int32_t tile_envs, int32_t grid, int32_t rollout_tile_envs) {
    if (!env) return fail(FE_ERR_ARG, "fe_env_set_launch: null env");
    if (tile_envs < 0 || grid < 0 || rollout_tile_envs < 0) return fail(FE_ERR_ARG, "fe_env_set_launch: negative value");
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    env->tile_override = tile_envs;
    env->grid_override = grid;
    env->rollout_tile_override = rollout_tile_envs;
    return configure_launch(env);
}

const char *fe_build_tag(void) { return FE_BUILD_TAG; }

int fe_env_destroy(fe_env *env) {
    if (env && (env->owned_logret || env->ticket)) {
        DeviceGuard guard(env->device);
        release_env(env);
    } else {
        delete env;
    }
    return FE_OK;
}

int fe_env_device(const fe_env *env) {
    if (!env) return fail(FE_ERR_ARG, "fe_env_device: null env");
    return env->device;
}

const double *fe_env_logret(const fe_env *env) { return env ? env->p.LR : nullptr; }

int fe_build_logret(const double *prices, double *out, int64_t T, int32_t A, void *stream) {
    if (!prices || !out || T < 1 || A < 1) return fail(FE_ERR_ARG, "fe_build_logret: bad argument");
    DeviceGuard guard(device_of(prices));
    if (int rc = guard.status()) return rc;
    hipLaunchKernelGGL(fe_logret_kernel, dim3(grid_for(T * A)), dim3(kBlock), 0, (hipStream_t)stream, prices, out, T, A);
    return launched("fe_build_logret");
}

int fe_build_logret_tables(const double *prices, double *out, int64_t D, int64_t L, int32_t A, void *stream) {
    if (!prices || !out || D < 1 || L < 1 || A < 1) return fail(FE_ERR_ARG, "fe_build_logret_tables: bad argument");
    DeviceGuard guard(device_of(prices));
    if (int rc = guard.status()) return rc;
    hipLaunchKernelGGL(fe_logret_tables_kernel, dim3(grid_for(D * L * A)), dim3(kBlock), 0, (hipStream_t)stream, prices,
                       out, D, L, A);
    return launched("fe_build_logret_tables");
}

int fe_build_tables(const double *series, const int64_t *starts, const int64_t *stops, int64_t D, int64_t L,
                    int32_t A, double *out, void *stream) {
    if (!series || !starts || !stops || !out || D < 1 || L < 1 || A < 1)
        return fail(FE_ERR_ARG, "fe_build_tables: bad argument");
    DeviceGuard guard(device_of(series));
    if (int rc = guard.status()) return rc;
    hipLaunchKernelGGL(fe_tables_kernel, dim3(grid_for(D * L * 4 * A)), dim3(kBlock), 0, (hipStream_t)stream, series,
                       starts, stops, D, L, A, out);
    return launched("fe_build_tables");
}

int fe_traj_store(int64_t t, int64_t N, int32_t A, const float *actions, const double *rewards,
                  const int32_t *dones, float *traj_actions, double *traj_rewards, int32_t *traj_dones,
                  void *stream) {
    if (t < 0 || N < 1 || A < 1 || !actions || !rewards || !dones || !traj_actions || !traj_rewards || !traj_dones)
        return fail(FE_ERR_ARG, "fe_traj_store: bad argument");
    DeviceGuard guard(device_of(traj_rewards));
    if (int rc = guard.status()) return rc;
    const int64_t NA = N * A;
    hipLaunchKernelGGL(fe_traj_store_kernel, dim3(grid_for(NA)), dim3(kBlock), 0, (hipStream_t)stream, N, NA, actions,
                       rewards, dones, traj_actions + t * NA, traj_rewards + t * N, traj_dones + t * N);
    return launched("fe_traj_store");
}

int fe_traj_returns(const double *rewards, const int32_t *dones, const float *values, const float *last_values,
                    int64_t T, int64_t N, double gamma, float *returns, float *advantages, void *stream) {
    if (!rewards || !dones || !last_values || !returns || T < 1 || N < 1 || (advantages && !values))
        return fail(FE_ERR_ARG, "fe_traj_returns: bad argument");
    DeviceGuard guard(device_of(rewards));
    if (int rc = guard.status()) return rc;
    // loads U steps ahead: U = 1 once the envs fill the chip on their own (fe_aux_kernels.h)
    with_bool(N >= (1 << 19), [&](auto full) {
        hipLaunchKernelGGL(fe_traj_returns_kernel<decltype(full)::value ? 1 : 4>, dim3(grid_for(N)), dim3(kBlock), 0,
                           (hipStream_t)stream, rewards, dones, values, last_values, T, N, (float)gamma, returns, advantages);
    });
    return launched("fe_traj_returns");
}

// ---- include/finenvs_amd_replay.h: the off-policy replay ring ----

static bool replay_ring_ok(const fe_replay_ring *ring) {
    return ring && ring->capacity >= 1 && ring->num_assets >= 1 && ring->state_src && ring->state_pos &&
           ring->next_src && ring->next_pos && ring->actions && ring->rewards && ring->dones && ring->errors;
}

static ReplayRing replay_view(const fe_replay_ring *ring) {
    ReplayRing r;
    r.s_src = ring->state_src; r.s_pos = ring->state_pos; r.n_src = ring->next_src; r.n_pos = ring->next_pos;
    r.act = ring->actions; r.rew = ring->rewards; r.done = ring->dones;
    r.C = ring->capacity; r.A = ring->num_assets;
    return r;
}

// fe_replay_append and fe_replay_append_c: the same kernel, `cursor` null for the by-value entry.
static int replay_append_impl(const fe_replay_ring *ring, int64_t head, int64_t steps, int64_t num_envs, int64_t row_stride,
                              int64_t first, int64_t count, const int64_t *state_src, const double *state_pos,
                              const int64_t *next_src, const double *next_pos, const void *actions, int32_t actions_are_f64,
                              const double *rewards, const int32_t *dones, int64_t *cursor, int64_t new_size, void *stream) {
    if (!replay_ring_ok(ring) || !state_src || !state_pos || !next_src || !next_pos || !actions || !rewards || !dones)
        return fail(FE_ERR_ARG, "fe_replay_append: null argument");
    const int64_t C = ring->capacity;
    if (steps < 1 || num_envs < 1 || row_stride < num_envs || first < 0 || count < 1 || count > C || head < 0 ||
        head >= C || first + count > steps * num_envs)
        return fail(FE_ERR_ARG, "fe_replay_append: bad range (steps %lld, num_envs %lld, row_stride %lld, first %lld, "
                    "count %lld, head %lld, capacity %lld)", (long long)steps, (long long)num_envs, (long long)row_stride,
                    (long long)first, (long long)count, (long long)head, (long long)C);
    if (cursor && (new_size < count || new_size > C))
        return fail(FE_ERR_ARG, "fe_replay_append_c: new_size %lld is not in [count %lld, capacity %lld]", (long long)new_size,
                    (long long)count, (long long)C);
    DeviceGuard guard(device_of(ring->rewards));
    if (int rc = guard.status("fe_replay_append: the ring is not device memory")) return rc;
    const ReplayRing r = replay_view(ring);
    with_bool(r.A == 1, [&](auto S) {
        with_bool(actions_are_f64 != 0, [&](auto F) {
            hipLaunchKernelGGL((fe_replay_append_kernel<decltype(S)::value, decltype(F)::value>), dim3(grid_for(count * r.A)),
                               dim3(kBlock), 0, (hipStream_t)stream, r, head, first, count, num_envs, row_stride, state_src,
                               state_pos, next_src, next_pos, actions, rewards, dones, cursor, new_size);
        });
    });
    return launched("fe_replay_append");
}

int fe_replay_append(const fe_replay_ring *ring, int64_t head, int64_t steps, int64_t num_envs, int64_t row_stride,
                     int64_t first, int64_t count, const int64_t *state_src, const double *state_pos,
                     const int64_t *next_src, const double *next_pos, const void *actions, int32_t actions_are_f64,
                     const double *rewards, const int32_t *dones, void *stream) {
    return replay_append_impl(ring, head, steps, num_envs, row_stride, first, count, state_src, state_pos, next_src, next_pos,
                              actions, actions_are_f64, rewards, dones, nullptr, 0, stream);
}

int fe_replay_append_c(const fe_replay_ring *ring, int64_t head, int64_t steps, int64_t num_envs, int64_t row_stride,
                       int64_t first, int64_t count, const int64_t *state_src, const double *state_pos,
                       const int64_t *next_src, const double *next_pos, const void *actions, int32_t actions_are_f64,
                       const double *rewards, const int32_t *dones, int64_t *cursor, int64_t new_size, void *stream) {
    if (!cursor) return fail(FE_ERR_ARG, "fe_replay_append_c: null cursor");
    return replay_append_impl(ring, head, steps, num_envs, row_stride, first, count, state_src, state_pos, next_src, next_pos,
                              actions, actions_are_f64, rewards, dones, cursor, new_size, stream);
}

int fe_ring_draw(const fe_replay_ring *ring, int64_t *cursor, uint64_t seed, int64_t count, int64_t *indices_out,
                 int64_t *state_src, double *state_pos, int64_t *next_src, double *next_pos, float *actions,
                 float *rewards, float *dones, void *stream) {
    if (!replay_ring_ok(ring) || !cursor || !indices_out || count < 0)
        return fail(FE_ERR_ARG, "fe_ring_draw: bad argument");
    if (ring->capacity >= (int64_t)1 << 32)
        return fail(FE_ERR_ARG, "fe_ring_draw: capacity %lld does not fit the 32-bit multiply-shift draw", (long long)ring->capacity);
    if (count == 0) return FE_OK;
    DeviceGuard guard(device_of(ring->rewards));
    if (int rc = guard.status("fe_ring_draw: the ring is not device memory")) return rc;
    RingDrawArgs d;
    d.r = replay_view(ring);
    d.errors = reinterpret_cast<unsigned long long *>(ring->errors);
    d.cursor = cursor; d.seed = seed; d.count = count; d.idx = indices_out;
    d.s_src = state_src; d.s_pos = state_pos; d.n_src = next_src; d.n_pos = next_pos;
    d.act = actions; d.rew = rewards; d.done = dones;
    hipLaunchKernelGGL(fe_ring_draw_kernel, dim3(grid_for(count * d.r.A)), dim3(kBlock), 0, (hipStream_t)stream, d);
    return launched("fe_ring_draw");
}

// fe_replay_sample and fe_replay_sample_c: the same kernel, `cursor` null for the by-value entry (head / size ignored
// and unchecked with a cursor: they are read on the device).
static int replay_sample_impl(fe_env *env, const fe_replay_ring *ring, int64_t head, int64_t size, const int64_t *cursor,
                              const int64_t *indices, int64_t count, float *states, float *next_states, float *actions,
                              float *rewards, float *dones, void *stream) {
    if (!env || !replay_ring_ok(ring) || !indices || !states || !next_states || !actions || !rewards || !dones || count < 0)
        return fail(FE_ERR_ARG, "fe_replay_sample: bad argument");
    const int64_t C = ring->capacity;
    if (!cursor && (size < 1 || size > C || head < 0 || head >= C))
        return fail(FE_ERR_ARG, "fe_replay_sample: size %lld / head %lld do not describe a non-empty ring of %lld slots",
                    (long long)size, (long long)head, (long long)C);
    if (ring->num_assets != env->p.A)
        return fail(FE_ERR_ARG, "fe_replay_sample: the ring holds %d assets, the env %d", (int)ring->num_assets,
                    (int)env->p.A);
    if (count == 0) return FE_OK;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    Params p = env->p;
    const int A = p.A;
    // Tile = EB samples.  A workgroup iteration of stream_tile<float> turns 4 x 256 tuples: a tile is a whole number of
    // them where the LDS allows (two descriptor tiles of EB (8 + 8A) bytes each, kept within 32 KiB), and there are
    // about four tiles per CU.
    int64_t cap = 2048 / (1 + A);
    if (cap < 1) cap = 1;
    const int64_t wg_tuples = 4 * (kStageBytes / 20);
    const int64_t unit = wg_tuples / std::gcd(wg_tuples, (int64_t)p.W * A);  // samples per whole workgroup iteration
    int64_t EB = (count + 4 * (int64_t)env->cus - 1) / (4 * (int64_t)env->cus);
    if (unit <= cap) EB = EB <= unit ? unit : EB - EB % unit;
    if (EB > cap) EB = cap;
    if (EB < 1) EB = 1;
    p.N = count;
    p.EB = (int32_t)EB;
    p.num_tiles = (count + EB - 1) / EB;
    p.obs_stream = 0;  // a minibatch is read by the learner right away: keep it in the Infinity Cache
    const int64_t grid = p.num_tiles < 8 * (int64_t)env->cus ? p.num_tiles : 8 * (int64_t)env->cus;
    const size_t lds = replay_lds_bytes((int)EB, A);
    const ReplayRing r = replay_view(ring);
    const int64_t start = cursor ? 0 : ((head - size) % C + C) % C;
    unsigned long long *err = reinterpret_cast<unsigned long long *>(ring->errors);
    // the sampled states are f32 observations
    with_layout(/*f32=*/true, vec_width(p.env_elems, 4), [&](auto, auto V) {
        with_bool(A == 1, [&](auto S) {
            hipLaunchKernelGGL((fe_replay_sample_kernel<decltype(V)::value, decltype(S)::value>), dim3((unsigned)grid),
                               dim3(kBlock), lds, (hipStream_t)stream, p, r, indices, start, size, states, next_states,
                               actions, rewards, dones, err, cursor);
        });
    });
    return launched("fe_replay_sample");
}

int fe_replay_sample(fe_env *env, const fe_replay_ring *ring, int64_t head, int64_t size, const int64_t *indices,
                     int64_t count, float *states, float *next_states, float *actions, float *rewards, float *dones,
                     void *stream) {
    return replay_sample_impl(env, ring, head, size, nullptr, indices, count, states, next_states, actions, rewards, dones,
                              stream);
}

int fe_replay_sample_c(fe_env *env, const fe_replay_ring *ring, const int64_t *cursor, const int64_t *indices,
                       int64_t count, float *states, float *next_states, float *actions, float *rewards, float *dones,
                       void *stream) {
    if (!cursor) return fail(FE_ERR_ARG, "fe_replay_sample_c: null cursor");
    return replay_sample_impl(env, ring, 0, 0, cursor, indices, count, states, next_states, actions, rewards, dones, stream);
}

// ---- include/finenvs_amd_critic.h and include/finenvs_amd_critic_streamed.h: the twin LSTM critics, their Bellman
// targets and, at H = 256 / 512 / 1024, their streamed forms ----
static bool critic_weights_ok(const fe_critic_weights *c) { return c && c->whh && c->wx && c->wout && c->bout; }

// The checks the critics' entries share; `env` is dereferenced only after the ones that need no env.
static int critic_check(const fe_env *env, int32_t H, bool streamed, const char *who) {
    if (streamed && !lstm_sgrad_hidden_ok(H))
        return fail(FE_ERR_ARG, "%s: H must be 256, 512 or 1024 (got %d); H = 32, 64 and 128 run the register-resident "
                    "entries of finenvs_amd_critic.h / finenvs_amd_critic_grad.h", who, (int)H);
    if (!streamed && !resident_h_ok(H))
        return fail(FE_ERR_ARG, "%s: H must be 32, 64 or 128 (got %d): the twin critic has no streamed or split kernel", who, (int)H);
    if (env->p.A != 1)
        return fail(FE_ERR_ARG, "%s: the env has %d assets; the fused critic runs A = 1 only (the reference's critic for A > 1 "
                    "is one nn.LSTM(5A + A, H) over the whole env, not a per-(env, asset) pair network)", who, (int)env->p.A);
    return streamed ? lds_fits(critic_sgrad_forward_lds_bytes(H), H, who) : FE_OK;
}

// Shared by fe_twin_q_forward and fe_twin_q_target: the split grid -- blockIdx.y = critic -- of fe_twin_q_kernel, each
// half at most half the resident workgroups, looping over all tiles.
static int launch_twin_q(fe_env *env, CriticArgs &cq, int64_t count, const char *who, void *stream) {
    const int32_t H = cq.l.H;
    Params p = env->p;
    p.eval_env = -1;
    const int SP = lstm_geometry(env, p, count, H, false, who);
    if (SP == 0) return FE_ERR_ARG;
    const size_t lds = lstm_lds_bytes(p.EB, p.A, H, SP);
    const void *kern = with_nt(H, [](auto NT) { return (const void *)fe_twin_q_kernel<decltype(NT)::value>; });
    int per_cu = 0;
    const hipError_t he = prepare_kernel(env->device, kern, kLstmBlock, lds, &per_cu);
    if (he != hipSuccess) return hip_fail(he, "twin critic kernel: hipFuncSetAttribute / occupancy query");
    int64_t half = (int64_t)env->cus * per_cu / 2;
    if (half < 1) half = 1;
    const int64_t grid = p.num_tiles < half ? p.num_tiles : half;
    void *args[] = {&p, &cq};
    return launched(who, hipLaunchKernel(kern, dim3((unsigned)grid, 2), dim3(kLstmBlock), args, lds, (hipStream_t)stream));
}

static void critic_args(CriticArgs &cq, const float *logret_f32, const fe_critic_weights *c1, const fe_critic_weights *c2,
                        int32_t H, float *q1_out, float *q2_out) {
    memset(&cq, 0, sizeof(cq));
    cq.l.lr32 = logret_f32; cq.l.H = H; cq.l.out_act = 2; cq.l.K = 1; cq.l.forward_only = 1;
    const fe_critic_weights *c[2] = {c1, c2};
    float *q[2] = {q1_out, q2_out};
    for (int i = 0; i < 2; ++i) cq.net[i] = CriticNet{c[i]->whh, c[i]->wx, c[i]->wout, c[i]->bout, q[i]};
}

// One launch of a streamed recurrence kernel (kLstmBlock threads, `a` its one argument) over `tiles` 32-pair tiles: at
// most the resident workgroups, each looping over its tiles.  `what` names the kernel in a preparation error, `step` the
// launch.
static int launch_sgrad_forward(const fe_env *env, const void *kern, size_t lds, void *a, int64_t tiles, const char *what,
                                const char *step, hipStream_t st) {
    int per_cu = 0;
    const hipError_t he = prepare_kernel(env->device, kern, kLstmBlock, lds, &per_cu);
    if (he != hipSuccess) return hip_fail(he, what);
    int64_t resident = (int64_t)env->cus * per_cu;
    if (resident < 1) resident = 1;
    void *args[] = {a};
    return launched(step, hipLaunchKernel(kern, dim3((unsigned)(tiles < resident ? tiles : resident)), dim3(kLstmBlock),
                                          args, lds, st));
}

static const char *const kCriticSGradPrepare = "streamed critic kernel: hipFuncSetAttribute / occupancy query";

// The streamed critics' recurrence kernel, without the stash (values, targets) or with it (backward).  Defined further
// down, where the code object has these instantiations: it lists them as the host code first names them (mlp_head_kernels).
static const void *critic_sgrad_kernel(int32_t H, bool stash);

// The streamed counterpart of launch_twin_q: the forward-only recurrence for both critics, one after the other (a:
// descriptors, actions and ring already set).
static int launch_twin_q_streamed(fe_env *env, CriticSGradArgs &a, const fe_critic_weights *c1, const fe_critic_weights *c2,
                                  int32_t H, int64_t count, float *q1_out, float *q2_out, const char *who, void *stream) {
    const void *kern = critic_sgrad_kernel(H, /*stash=*/false);
    const fe_critic_weights *c[2] = {c1, c2};
    float *q[2] = {q1_out, q2_out};
    a.g.W = env->p.W; a.g.cnt = count; a.g.pp = (count + 31) / 32 * 32;
    for (int i = 0; i < 2; ++i) {
        a.g.whh = c[i]->whh; a.g.wx = c[i]->wx; a.g.wout = c[i]->wout; a.bout = c[i]->bout; a.q_out = q[i];
        if (int rc = launch_sgrad_forward(env, kern, critic_sgrad_forward_lds_bytes(H), &a, a.g.pp / 32, kCriticSGradPrepare, who,
                                          (hipStream_t)stream))
            return rc;
    }
    return FE_OK;
}

// fe_twin_q_forward and fe_twin_q_forward_streamed
static int twin_q_forward_impl(fe_env *env, const float *logret_f32, const fe_critic_weights *c1, const fe_critic_weights *c2,
                               int32_t H, const int64_t *obs_src, const double *obs_pos, const float *actions, int64_t count,
                               float *q1_out, float *q2_out, void *stream, bool streamed, const char *who) {
    if (!env || !logret_f32 || !critic_weights_ok(c1) || !critic_weights_ok(c2) || !obs_src || !obs_pos || !actions ||
        !q1_out || !q2_out || count < 0)
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (int rc = critic_check(env, H, streamed, who)) return rc;
    if (count == 0) return FE_OK;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    if (streamed) {
        CriticSGradArgs a;
        memset(&a, 0, sizeof(a));
        a.g.lr32 = logret_f32; a.g.obs_src = obs_src; a.g.obs_pos = obs_pos; a.actions = actions;
        return launch_twin_q_streamed(env, a, c1, c2, H, count, q1_out, q2_out, who, stream);
    }
    CriticArgs cq;
    critic_args(cq, logret_f32, c1, c2, H, q1_out, q2_out);
    cq.l.obs_src = const_cast<int64_t *>(obs_src); cq.l.obs_pos = const_cast<double *>(obs_pos);  // read only in this mode
    cq.actions = actions;
    return launch_twin_q(env, cq, count, who, stream);
}

int fe_twin_q_forward(fe_env *env, const float *logret_f32, const fe_critic_weights *c1, const fe_critic_weights *c2,
                      int32_t H, const int64_t *obs_src, const double *obs_pos, const float *actions, int64_t count,
                      float *q1_out, float *q2_out, void *stream) {
    return twin_q_forward_impl(env, logret_f32, c1, c2, H, obs_src, obs_pos, actions, count, q1_out, q2_out, stream, false,
                               "fe_twin_q_forward");
}

int fe_twin_q_forward_streamed(fe_env *env, const float *logret_f32, const fe_critic_weights *c1,
                               const fe_critic_weights *c2, int32_t H, const int64_t *obs_src, const double *obs_pos,
                               const float *actions, int64_t count, float *q1_out, float *q2_out, void *stream) {
    return twin_q_forward_impl(env, logret_f32, c1, c2, H, obs_src, obs_pos, actions, count, q1_out, q2_out, stream, true,
                               "fe_twin_q_forward_streamed");
}

// fe_twin_q_target, fe_twin_q_target_streamed and their _c forms: `cursor` null for a by-value entry (head / size ignored
// and unchecked with a cursor: they are read on the device).  `who`: "fe_twin_q_target" or "fe_twin_q_target_streamed".
static int twin_q_target_impl(fe_env *env, const float *logret_f32, const fe_critic_weights *c1, const fe_critic_weights *c2,
                              int32_t H, const fe_replay_ring *ring, int64_t head, int64_t size, const int64_t *cursor,
                              const int64_t *indices, int64_t count, const float *next_actions, const float *smooth_noise,
                              float smooth_std, float smooth_clip, const float *log_probs, const float *alpha, float gamma,
                              float reward_scale, float *targets_out, float *q1_out, float *q2_out, void *stream,
                              bool streamed, const char *who) {
    if (!env || !logret_f32 || !critic_weights_ok(c1) || !critic_weights_ok(c2) || !replay_ring_ok(ring) || !indices ||
        !next_actions || !targets_out || !q1_out || !q2_out || count < 0)
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (log_probs && !alpha) return fail(FE_ERR_ARG, "%s: log_probs (SAC) need alpha", who);
    if (smooth_noise && log_probs)
        return fail(FE_ERR_ARG, "%s: smooth_noise (TD3) and log_probs (SAC) are exclusive", who);
    if (int rc = critic_check(env, H, streamed, who)) return rc;
    const int64_t C = ring->capacity;
    if (!cursor && (size < 1 || size > C || head < 0 || head >= C))
        return fail(FE_ERR_ARG, "%s: size %lld / head %lld do not describe a non-empty ring of %lld slots", who,
                    (long long)size, (long long)head, (long long)C);
    if (ring->num_assets != 1) return fail(FE_ERR_ARG, "%s: the ring holds %d assets, the env 1", who, (int)ring->num_assets);
    if (count == 0) return FE_OK;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    const int64_t start = cursor ? 0 : ((head - size) % C + C) % C;
    const auto sampled = [&](auto &x) {  // the next states' descriptors in the ring and the actions taken there
        x.indices = indices; x.ring_src = ring->next_src; x.ring_pos = ring->next_pos;
        x.ring_C = C; x.start = start; x.size = size; x.cursor = cursor;
        x.actions = next_actions; x.smooth_noise = smooth_noise; x.smooth_std = smooth_std; x.smooth_clip = smooth_clip;
    };
    if (streamed) {
        CriticSGradArgs a;
        memset(&a, 0, sizeof(a));
        a.g.lr32 = logret_f32;
        sampled(a);
        if (int rc = launch_twin_q_streamed(env, a, c1, c2, H, count, q1_out, q2_out, "fe_twin_q_target_streamed: critics", stream))
            return rc;
    } else {
        CriticArgs cq;
        critic_args(cq, logret_f32, c1, c2, H, q1_out, q2_out);
        sampled(cq);
        if (int rc = launch_twin_q(env, cq, count, "fe_twin_q_target: critics", stream)) return rc;
    }
    TwinTargetArgs t;
    t.q1 = q1_out; t.q2 = q2_out; t.indices = indices; t.ring_rew = ring->rewards; t.ring_done = ring->dones;
    t.ring_C = C; t.start = start; t.size = size; t.count = count; t.log_probs = log_probs; t.alpha = alpha;
    t.gamma = gamma; t.reward_scale = reward_scale; t.targets = targets_out;
    t.errors = reinterpret_cast<unsigned long long *>(ring->errors);
    t.cursor = cursor;
    hipLaunchKernelGGL(fe_twin_q_target_kernel, dim3(grid_for(count)), dim3(kBlock), 0, (hipStream_t)stream, t);
    return launched(streamed ? "fe_twin_q_target_streamed: epilogue" : "fe_twin_q_target: epilogue");
}

int fe_twin_q_target(fe_env *env, const float *logret_f32, const fe_critic_weights *c1, const fe_critic_weights *c2,
                     int32_t H, const fe_replay_ring *ring, int64_t head, int64_t size, const int64_t *indices,
                     int64_t count, const float *next_actions, const float *smooth_noise, float smooth_std,
                     float smooth_clip, const float *log_probs, const float *alpha, float gamma, float reward_scale,
                     float *targets_out, float *q1_out, float *q2_out, void *stream) {
    return twin_q_target_impl(env, logret_f32, c1, c2, H, ring, head, size, nullptr, indices, count, next_actions,
                              smooth_noise, smooth_std, smooth_clip, log_probs, alpha, gamma, reward_scale, targets_out,
                              q1_out, q2_out, stream, false, "fe_twin_q_target");
}

int fe_twin_q_target_c(fe_env *env, const float *logret_f32, const fe_critic_weights *c1, const fe_critic_weights *c2,
                       int32_t H, const fe_replay_ring *ring, const int64_t *cursor, const int64_t *indices,
                       int64_t count, const float *next_actions, const float *smooth_noise, float smooth_std,
                       float smooth_clip, const float *log_probs, const float *alpha, float gamma, float reward_scale,
                       float *targets_out, float *q1_out, float *q2_out, void *stream) {
    if (!cursor) return fail(FE_ERR_ARG, "fe_twin_q_target_c: null cursor");
    return twin_q_target_impl(env, logret_f32, c1, c2, H, ring, 0, 0, cursor, indices, count, next_actions, smooth_noise,
                              smooth_std, smooth_clip, log_probs, alpha, gamma, reward_scale, targets_out, q1_out, q2_out,
                              stream, false, "fe_twin_q_target");
}

int fe_twin_q_target_streamed(fe_env *env, const float *logret_f32, const fe_critic_weights *c1,
                              const fe_critic_weights *c2, int32_t H, const fe_replay_ring *ring, int64_t head,
                              int64_t size, const int64_t *indices, int64_t count, const float *next_actions,
                              const float *smooth_noise, float smooth_std, float smooth_clip, const float *log_probs,
                              const float *alpha, float gamma, float reward_scale, float *targets_out, float *q1_out,
                              float *q2_out, void *stream) {
    return twin_q_target_impl(env, logret_f32, c1, c2, H, ring, head, size, nullptr, indices, count, next_actions,
                              smooth_noise, smooth_std, smooth_clip, log_probs, alpha, gamma, reward_scale, targets_out,
                              q1_out, q2_out, stream, true, "fe_twin_q_target_streamed");
}

int fe_twin_q_target_streamed_c(fe_env *env, const float *logret_f32, const fe_critic_weights *c1,
                                const fe_critic_weights *c2, int32_t H, const fe_replay_ring *ring, const int64_t *cursor,
                                const int64_t *indices, int64_t count, const float *next_actions,
                                const float *smooth_noise, float smooth_std, float smooth_clip, const float *log_probs,
                                const float *alpha, float gamma, float reward_scale, float *targets_out, float *q1_out,
                                float *q2_out, void *stream) {
    if (!cursor) return fail(FE_ERR_ARG, "fe_twin_q_target_streamed_c: null cursor");
    return twin_q_target_impl(env, logret_f32, c1, c2, H, ring, 0, 0, cursor, indices, count, next_actions, smooth_noise,
                              smooth_std, smooth_clip, log_probs, alpha, gamma, reward_scale, targets_out, q1_out, q2_out,
                              stream, true, "fe_twin_q_target_streamed");
}

// ---- what the streamed backward passes (head, twin critics, SAC actor at H = 256 / 512 / 1024) share ----
// wt | part | hpart | gates from the workspace: the layout of fe_lstm_streamed_grad_workspace_floats, sized by the largest
// pass (pp pairs).  g.W is set.
static void sgrad_carve(LstmSGradArgs &g, float *workspace, int32_t H, int64_t pp) {
    g.wt = workspace;
    g.part = g.wt + lstm_sgrad_wt_floats(H);
    g.hpart = g.part + lstm_sgrad_splits(H, g.W, pp) * lstm_sgrad_part_floats(H);
    g.gates = g.hpart + lstm_sgrad_head_blocks(pp) * (H + 32);
}

// A chunk after its recurrence: head -> (dz [, dh]) x W -> [d_actions] -> [weight contraction -> final write], every launch
// reported as "<who>: <stage>".  `da`: the critic's argument block around g when d_actions are wanted, else null.
// `final_kernel` null: a frozen critic.
// `sac`: the SAC actor's argument block around g (g IS sac->g): its head stages (z, head, dh_W) replace the one-output
// head's, its last-layer contraction follows the LSTM's and its final kernel writes all ten tensors (final_kernel unused).
static int sgrad_backward_chunk(const char *who, LstmSGradArgs &g, int32_t H, const CriticSGradArgs *da,
                                void (*final_kernel)(LstmSGradArgs, int32_t), hipStream_t st, const SacSGradArgs *sac) {
    const int W = g.W;
    const int64_t tiles = g.pp / 32;
    if (sac) {
        hipLaunchKernelGGL(fe_sac_sgrad_z_kernel, dim3((unsigned)(H / 128), (unsigned)tiles), dim3(kBlock), 0, st, *sac, H);
        if (int rc = launched(who, "last layer")) return rc;
        hipLaunchKernelGGL(fe_sac_sgrad_head_kernel, dim3((unsigned)lstm_sgrad_head_blocks(g.pp)), dim3(kBlock), 0, st, *sac, H);
        hipLaunchKernelGGL(fe_sac_sgrad_dh_kernel, dim3((unsigned)(H / kLstmSGradDhUnits), (unsigned)tiles), dim3(kBlock), 0,
                           st, *sac, H);
    } else {
        hipLaunchKernelGGL(fe_lstm_sgrad_head_kernel, dim3((unsigned)lstm_sgrad_head_blocks(g.pp)), dim3(kBlock), 0, st, g, H);
    }
    if (int rc = launched(who, "head")) return rc;
    for (int t = W - 1; t >= 0; --t) {
        g.t = t;
        hipLaunchKernelGGL(fe_lstm_sgrad_dz_kernel, dim3(grid_for(g.pp * (H / 4))), dim3(kBlock), 0, st, g, H);
        if (t > 0)
            hipLaunchKernelGGL(fe_lstm_sgrad_dh_kernel, dim3((unsigned)(H / kLstmSGradDhUnits), (unsigned)tiles),
                               dim3(kBlock), 0, st, g, H);
        // a launch that fails fails the first time: stop before queueing 2 W launches behind it
        if (t == W - 1) {
            if (int rc = launched(who, "backward through time")) return rc;
        }
    }
    if (da) {
        const int64_t blocks = (g.cnt + kBlock / 64 - 1) / (kBlock / 64);
        hipLaunchKernelGGL(fe_critic_sgrad_da_kernel, dim3((unsigned)capped_grid(blocks)), dim3(kBlock),
                           (size_t)4 * H * sizeof(float), st, *da, H);
        if (int rc = launched(who, "d_actions")) return rc;
    }
    if (!final_kernel && !sac) return FE_OK;  // frozen: no weight contraction, no final write
    hipLaunchKernelGGL(fe_lstm_sgrad_wgrad_kernel,
                       dim3((unsigned)(4 * H / kLstmSGradWgRows * ((H + 32) / 32)), (unsigned)g.splits), dim3(kBlock), 0,
                       st, g, H);
    if (int rc = launched(who, "weight gradients")) return rc;
    if (sac) {
        hipLaunchKernelGGL(fe_sac_sgrad_wl_kernel, dim3((unsigned)(H / kLstmSGradWgRows * (H / 32)), (unsigned)sac->wl_splits),
                           dim3(kBlock), 0, st, *sac, H);
        if (int rc = launched(who, "last layer weight gradients")) return rc;
        hipLaunchKernelGGL(fe_sac_sgrad_final_kernel, dim3(grid_for(lstm_sgrad_part_floats(H))), dim3(kBlock), 0, st, *sac, H);
        return launched(who, "final write");
    }
    hipLaunchKernelGGL(final_kernel, dim3(grid_for(lstm_sgrad_part_floats(H))), dim3(kBlock), 0, st, g, H);
    return launched(who, "final write");
}

// A streamed backward pass over `count` pairs, chunk by chunk in ascending order: the first chunk overwrites the
// gradients, the later ones add to them.  Per chunk: g's sizes, its buffers behind g.gates and its descriptors, then what
// `at(c0)` points the caller's own per-pair arrays at, the recurrence (`kern` on `fwd`, which is g or the argument block
// around it; `what` names the kernel in a preparation error) and sgrad_backward_chunk with `da`, `final_kernel`, `sac`.
extern "C++" {  // (a template)
template <class F>
static int sgrad_chunks(const fe_env *env, const char *who, LstmSGradArgs &g, int32_t H, int64_t count, const int64_t *obs_src,
                        const double *obs_pos, const void *kern, size_t lds, void *fwd, const char *what,
                        const CriticSGradArgs *da, void (*final_kernel)(LstmSGradArgs, int32_t), const SacSGradArgs *sac,
                        hipStream_t st, F &&at) {
    char step[64];
    snprintf(step, sizeof(step), "%s: recurrence", who);
    const int64_t W = g.W, chunk = lstm_sgrad_chunk_pairs(H, g.W);
    for (int64_t c0 = 0; c0 < count; c0 += chunk) {
        g.cnt = count - c0 < chunk ? count - c0 : chunk;
        g.pp = (g.cnt + 31) / 32 * 32;  // the last chunk may be shorter: same buffers, fewer rows of them
        g.splits = lstm_sgrad_splits(H, g.W, g.pp);
        g.cst = g.gates + W * g.pp * 4 * H;
        g.vst = g.cst + W * g.pp * H;
        g.hw = g.vst + W * g.pp * (H + 32);
        g.dh = g.hw + g.pp * H;
        g.dc = g.dh + g.pp * H;
        g.first = c0 == 0;
        g.obs_src = obs_src + c0; g.obs_pos = obs_pos + c0;
        at(c0);
        if (int rc = launch_sgrad_forward(env, kern, lds, fwd, g.pp / 32, what, step, st)) return rc;
        if (int rc = sgrad_backward_chunk(who, g, H, da, final_kernel, st, sac)) return rc;
    }
    return FE_OK;
}
}  // extern "C++"

// ---- include/finenvs_amd_critic_grad.h and the backward entry of include/finenvs_amd_critic_streamed.h ----
// Workspace: [wt of each critic][partials of each critic][stash of each critic][da of each critic].
int64_t fe_twin_q_grad_workspace_floats(int32_t H, int32_t W, int64_t count) {
    if (!resident_h_ok(H) || W < 1 || count < 0) return -1;
    const int64_t groups = grad_tiles(count, critic_grad_max_groups(H)).max_groups;
    return 2 * (critic_grad_wt_floats(H) + groups * (critic_grad_part_floats(H) + bptt_stash_floats(H, W))) +
           2 * count;
}

// The workspace of fe_lstm_backward_streamed, used by one critic after the other; d_actions is written in place.
int64_t fe_twin_q_streamed_grad_workspace_floats(int32_t H, int32_t W, int64_t count) {
    return fe_lstm_streamed_grad_workspace_floats(H, W, count);
}

// fe_twin_q_backward and fe_twin_q_backward_streamed.  A critic without dq takes no part; one without grads is frozen
// and only passes d_actions on.
static int twin_q_backward_impl(fe_env *env, const float *logret_f32, const fe_critic_weights *c1, const fe_critic_weights *c2,
                                int32_t H, const int64_t *obs_src, const double *obs_pos, const float *actions, int64_t count,
                                const float *dq1, const float *dq2, float *workspace, const fe_critic_grads *grads1,
                                const fe_critic_grads *grads2, float *d_actions, void *stream, bool streamed, const char *who) {
    if (!env || !logret_f32 || !obs_src || !obs_pos || !actions || !workspace || count < 0 ||
        (dq1 && (!critic_weights_ok(c1) || (grads1 && !head_grads_given(grads1)) || (!grads1 && !d_actions))) ||
        (dq2 && (!critic_weights_ok(c2) || (grads2 && !head_grads_given(grads2)) || (!grads2 && !d_actions))))
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (streamed) {
        if (int rc = critic_check(env, H, true, who)) return rc;
    } else {  // (the resident entry words its two refusals more briefly than critic_check)
        if (!resident_h_ok(H)) return fail(FE_ERR_ARG, "%s: H must be 32, 64 or 128 (got %d)", who, (int)H);
        if (env->p.A != 1)
            return fail(FE_ERR_ARG, "%s: the env has %d assets; the fused critic runs A = 1 only", who, (int)env->p.A);
    }
    if (count == 0) return FE_OK;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const fe_critic_weights *cw[2];
    const fe_critic_grads *cg[2];
    const float *dq[2];
    int ncrit = 0;  // the critics that take part, in order
    if (dq1) { cw[ncrit] = c1; cg[ncrit] = grads1; dq[ncrit++] = dq1; }
    if (dq2) { cw[ncrit] = c2; cg[ncrit] = grads2; dq[ncrit++] = dq2; }
    if (ncrit == 0) {
        if (!d_actions) return FE_OK;
        return launched(who, hipMemsetAsync(d_actions, 0, (size_t)count * sizeof(float), st));
    }
    const int W = env->p.W;
    if (streamed) {
        const int64_t pp = lstm_sgrad_padded_pairs(H, W, count);
        const void *kern = critic_sgrad_kernel(H, /*stash=*/true);
        for (int i = 0; i < ncrit; ++i) {
            CriticSGradArgs a;
            memset(&a, 0, sizeof(a));
            LstmSGradArgs &g = a.g;
            g.lr32 = logret_f32; g.whh = cw[i]->whh; g.wx = cw[i]->wx; g.wout = cw[i]->wout; g.W = W; g.out_act = 2;
            sgrad_carve(g, workspace, H, pp);
            if (cg[i]) head_grads_into(g, *cg[i]);
            a.da_add = d_actions && i > 0;  // a critic before this one has written d_actions
            hipLaunchKernelGGL(fe_lstm_sgrad_pack_kernel, dim3(grid_for(lstm_sgrad_wt_floats(H))), dim3(kBlock), 0, st, g, H);
            if (int rc = launched(who, "weight transpose")) return rc;
            const int rc = sgrad_chunks(env, who, g, H, count, obs_src, obs_pos, kern, critic_sgrad_forward_lds_bytes(H), &a,
                                        kCriticSGradPrepare, d_actions ? &a : nullptr,
                                        cg[i] ? fe_critic_sgrad_final_kernel : nullptr, nullptr, st, [&](int64_t c0) {
                                            g.d_outputs = dq[i] + c0;
                                            a.actions = actions + c0;
                                            a.da = d_actions ? d_actions + c0 : nullptr;
                                        });
            if (rc) return rc;
        }
        return FE_OK;
    }
    const auto [tiles, max_groups] = grad_tiles(count, critic_grad_max_groups(H));
    CriticGradArgs g;
    memset(&g, 0, sizeof(g));
    g.lr32 = logret_f32; g.obs_src = obs_src; g.obs_pos = obs_pos; g.actions = actions;
    g.count = count; g.num_tiles = tiles; g.W = W; g.d_actions = d_actions;
    float *wt = workspace, *part = wt + 2 * critic_grad_wt_floats(H);
    float *stash = part + 2 * max_groups * critic_grad_part_floats(H);
    float *da = stash + 2 * max_groups * bptt_stash_floats(H, W);
    g.ncrit = ncrit;
    for (int i = 0; i < ncrit; ++i) {
        CriticGradNet &n = g.net[i];
        n.whh = cw[i]->whh; n.wx = cw[i]->wx; n.wout = cw[i]->wout; n.dq = dq[i];
        n.wt = wt + i * critic_grad_wt_floats(H);
        n.part = part + i * max_groups * critic_grad_part_floats(H);
        n.stash = stash + i * max_groups * bptt_stash_floats(H, W);
        n.da = da + i * count;
        if (cg[i]) head_grads_into(n, *cg[i]);
    }
    hipLaunchKernelGGL(fe_critic_grad_pack_kernel, dim3(grid_for(critic_grad_wt_floats(H)), g.ncrit), dim3(kBlock), 0,
                       (hipStream_t)stream, g, H, const_cast<float *>(g.net[0].wt), const_cast<float *>(g.net[1].wt));
    if (int rc = launched("fe_twin_q_backward: weight transpose")) return rc;
    const void *kern = with_nt(H, [](auto NT) { return (const void *)fe_critic_grad_kernel<decltype(NT)::value>; });
    if (int rc = launch_grad(env, kern, critic_grad_lds_bytes(H), max_groups, g.ncrit, &g, &g.groups,
                             "critic gradient kernel: hipFuncSetAttribute / occupancy query", "fe_twin_q_backward: backward",
                             stream))
        return rc;
    const int64_t elems = 4LL * H * (H + 32) + H + 1;
    const int64_t work = elems > count ? elems : count;
    hipLaunchKernelGGL(fe_critic_grad_reduce_kernel, dim3(grid_for(work), g.ncrit + 1), dim3(kBlock), 0, (hipStream_t)stream,
                       g, H);
    return launched("fe_twin_q_backward: reduction");
}

int fe_twin_q_backward(fe_env *env, const float *logret_f32, const fe_critic_weights *c1, const fe_critic_weights *c2,
                       int32_t H, const int64_t *obs_src, const double *obs_pos, const float *actions, int64_t count,
                       const float *dq1, const float *dq2, float *workspace, const fe_critic_grads *grads1,
                       const fe_critic_grads *grads2, float *d_actions, void *stream) {
    return twin_q_backward_impl(env, logret_f32, c1, c2, H, obs_src, obs_pos, actions, count, dq1, dq2, workspace, grads1,
                                grads2, d_actions, stream, false, "fe_twin_q_backward");
}

int fe_twin_q_backward_streamed(fe_env *env, const float *logret_f32, const fe_critic_weights *c1,
                                const fe_critic_weights *c2, int32_t H, const int64_t *obs_src, const double *obs_pos,
                                const float *actions, int64_t count, const float *dq1, const float *dq2,
                                float *workspace, const fe_critic_grads *grads1, const fe_critic_grads *grads2,
                                float *d_actions, void *stream) {
    return twin_q_backward_impl(env, logret_f32, c1, c2, H, obs_src, obs_pos, actions, count, dq1, dq2, workspace, grads1,
                                grads2, d_actions, stream, true, "fe_twin_q_backward_streamed");
}

// ---- include/finenvs_amd_sac_grad.h: the SAC actor's backward pass ----
// Workspace: [W_hh^T | W_l^T][partials of every workgroup][stash of every workgroup].
int64_t fe_sac_grad_workspace_floats(int32_t H, int32_t W, int64_t count) {
    if (!resident_h_ok(H) || W < 1 || count < 0) return -1;
    const int64_t groups = grad_tiles(count, sac_grad_max_groups(H)).max_groups;
    return sac_grad_wt_floats(H) + groups * (sac_grad_part_floats(H) + bptt_stash_floats(H, W));
}

// The streamed SAC entries' refusal of another H; `small` names the entry that runs H = 32, 64 and 128.
static int sac_streamed_hidden(int32_t H, const char *who, const char *small) {
    if (lstm_sgrad_hidden_ok(H)) return FE_OK;
    return fail(FE_ERR_ARG, "%s: H must be 256, 512 or 1024 (got %d); %s runs H = 32, 64 and 128", who, (int)H, small);
}

// What fe_sac_backward (and its _p sibling) and fe_sac_backward_streamed refuse before they look at count; their launch
// sequences share nothing and stay with the entries.
static int sac_backward_checked(const fe_env *env, const float *logret_f32, const SacActorView &w, int32_t H,
                                const int64_t *obs_src, const double *obs_pos, int64_t count, const float *noise,
                                const float *actions, const float *stds, const float *d_actions, const float *d_log_probs,
                                const float *workspace, const fe_sac_grads *grads, bool streamed, const char *who) {
    if (!env || !logret_f32 || !sac_view_given(w) || !obs_src || !obs_pos || count < 0 || !noise || !actions || !stds ||
        (!d_actions && !d_log_probs) || !workspace || !grads || !grads->w_ih || !grads->w_hh || !grads->b_ih || !grads->b_hh ||
        !grads->w_l || !grads->b_l || !grads->w_mu || !grads->b_mu || !grads->w_std || !grads->b_std)
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (streamed) {
        if (int rc = sac_streamed_hidden(H, who, "fe_sac_backward")) return rc;
    } else if (!resident_h_ok(H)) {
        return fail(FE_ERR_ARG, "%s: H must be 32, 64 or 128 (got %d)", who, (int)H);
    }
    if (env->p.A != 1)
        return fail(FE_ERR_ARG, "%s: the env has %d assets; the fused actor gradient runs A = 1 only (its consumer, the "
                    "fused twin critic, does)", who, (int)env->p.A);
    return FE_OK;
}

// fe_sac_backward and fe_sac_backward_p (the gradient does not depend on bmu)
static int sac_backward_impl(fe_env *env, const float *logret_f32, const SacActorView &w, int32_t H, const int64_t *obs_src,
                             const double *obs_pos, int64_t count, const float *noise, const float *actions,
                             const float *stds, const float *d_actions, const float *d_log_probs, float *workspace,
                             const fe_sac_grads *grads, void *stream) {
    static const char *who = "fe_sac_backward";
    if (int rc = sac_backward_checked(env, logret_f32, w, H, obs_src, obs_pos, count, noise, actions, stds, d_actions,
                                      d_log_probs, workspace, grads, false, who))
        return rc;
    if (count == 0) return FE_OK;
    const size_t lds = sac_grad_lds_bytes(H);
    if (int rc = lds_fits(lds, H, who)) return rc;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    const int W = env->p.W;
    const auto [tiles, max_groups] = grad_tiles(count, sac_grad_max_groups(H));
    SacGradArgs g;
    memset(&g, 0, sizeof(g));
    g.lr32 = logret_f32; g.obs_src = obs_src; g.obs_pos = obs_pos;
    g.whh = w.whh; g.wx = w.wx; g.wl = w.wl; g.bl = w.bl; g.wmu = w.wmu; g.wstd = w.wstd; g.bstd = w.bstd; g.bstd_p = w.bstd_p;
    g.noise = noise; g.actions = actions; g.stds = stds; g.d_actions = d_actions; g.d_log_probs = d_log_probs;
    g.wt = workspace;
    g.part = g.wt + sac_grad_wt_floats(H);
    g.stash = g.part + max_groups * sac_grad_part_floats(H);
    g.count = count; g.num_tiles = tiles; g.W = W;
    g.g_wih = grads->w_ih; g.g_whh = grads->w_hh; g.g_bih = grads->b_ih; g.g_bhh = grads->b_hh; g.g_wl = grads->w_l;
    g.g_bl = grads->b_l; g.g_wmu = grads->w_mu; g.g_bmu = grads->b_mu; g.g_wstd = grads->w_std; g.g_bstd = grads->b_std;
    hipLaunchKernelGGL(fe_sac_grad_pack_kernel, dim3(grid_for(sac_grad_wt_floats(H))), dim3(kBlock), 0, (hipStream_t)stream,
                       g, H);
    if (int rc = launched("fe_sac_backward: weight transpose")) return rc;
    const void *kern = with_nt(H, [](auto NT) { return (const void *)fe_sac_grad_kernel<decltype(NT)::value>; });
    if (int rc = launch_grad(env, kern, lds, max_groups, 1, &g, &g.groups,
                             "SAC gradient kernel: hipFuncSetAttribute / occupancy query", "fe_sac_backward: backward", stream))
        return rc;
    hipLaunchKernelGGL(fe_sac_grad_reduce_kernel, dim3(grid_for(sac_grad_part_floats(H))), dim3(kBlock), 0,
                       (hipStream_t)stream, g, H);
    return launched("fe_sac_backward: reduction");
}

int fe_sac_backward(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                    const float *bl, const float *wmu, float bmu, const float *wstd, float bstd, int32_t H,
                    const int64_t *obs_src, const double *obs_pos, int64_t count, const float *noise,
                    const float *actions, const float *stds, const float *d_actions, const float *d_log_probs,
                    float *workspace, const fe_sac_grads *grads, void *stream) {
    return sac_backward_impl(env, logret_f32, {whh, wx, wl, bl, wmu, wstd, bmu, bstd, nullptr, nullptr}, H, obs_src, obs_pos,
                             count, noise, actions, stds, d_actions, d_log_probs, workspace, grads, stream);
}

// ---- include/finenvs_amd_lstm_grad.h and include/finenvs_amd_lstm_grad_streamed.h: the one-output LSTM head's backward
// pass, register-resident and streamed ----
// Workspace: [W_hh^T][partials of every workgroup][stash of every workgroup].
int64_t fe_lstm_grad_workspace_floats(int32_t H, int32_t W, int64_t count) {
    if (!resident_h_ok(H) || W < 1 || count < 0) return -1;
    const int64_t groups = grad_tiles(count, lstm_grad_max_groups(H)).max_groups;
    return lstm_grad_wt_floats(H) + groups * (lstm_grad_part_floats(H) + bptt_stash_floats(H, W));
}

// What fe_lstm_backward and fe_lstm_backward_streamed refuse before they look at count; their launch sequences share
// nothing and stay with the entries.
static int lstm_backward_checked(const fe_env *env, const float *logret_f32, const LstmHeadView &w, int32_t H,
                                 int32_t out_activation, const int64_t *obs_src, const double *obs_pos, int64_t count,
                                 const float *outputs, const float *d_outputs, const float *workspace,
                                 const fe_lstm_grads *grads, bool streamed, const char *who) {
    if (!env || !logret_f32 || !lstm_view_given(w) || !obs_src || !obs_pos || count < 0 || !d_outputs || !workspace ||
        !head_grads_given(grads))
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (out_activation != 0 && out_activation != 2)
        return fail(FE_ERR_ARG, "%s: out_activation must be 0 (tanh) or 2 (none); 1 (clamp) has no gradient to train on "
                    "(got %d)", who, (int)out_activation);
    if (out_activation == 0 && !outputs)
        return fail(FE_ERR_ARG, "%s: out_activation 0 (tanh) needs outputs, the values fe_lstm_forward returned", who);
    if (streamed && !lstm_sgrad_hidden_ok(H))
        return fail(FE_ERR_ARG, "%s: H must be 256, 512 or 1024 (got %d); fe_lstm_backward runs H = 32, 64 and 128", who,
                    (int)H);
    if (!streamed && !resident_h_ok(H))
        return fail(FE_ERR_ARG, "%s: H must be 32, 64 or 128 (got %d): the streamed-weight forward of H >= 256 has no "
                    "register-resident recurrence to mirror", who, (int)H);
    if (env->p.A != 1)
        return fail(FE_ERR_ARG, "%s: the env has %d assets; the fused head gradient runs A = 1 only (as the fused twin "
                    "critic does)", who, (int)env->p.A);
    return FE_OK;
}

int fe_lstm_backward(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wout,
                     int32_t H, int32_t out_activation, const int64_t *obs_src, const double *obs_pos, int64_t count,
                     const float *outputs, const float *d_outputs, float *workspace, const fe_lstm_grads *grads,
                     void *stream) {
    static const char *who = "fe_lstm_backward";
    if (int rc = lstm_backward_checked(env, logret_f32, {whh, wx, wout, 0.0f, nullptr}, H, out_activation, obs_src, obs_pos,
                                       count, outputs, d_outputs, workspace, grads, false, who))
        return rc;
    if (count == 0) return FE_OK;
    const size_t lds = lstm_grad_lds_bytes(H);
    if (int rc = lds_fits(lds, H, who)) return rc;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    const int W = env->p.W;
    const auto [tiles, max_groups] = grad_tiles(count, lstm_grad_max_groups(H));
    LstmGradArgs g;
    memset(&g, 0, sizeof(g));
    g.lr32 = logret_f32; g.obs_src = obs_src; g.obs_pos = obs_pos;
    g.whh = whh; g.wx = wx; g.wout = wout; g.outputs = outputs; g.d_outputs = d_outputs;
    g.wt = workspace;
    g.part = g.wt + lstm_grad_wt_floats(H);
    g.stash = g.part + max_groups * lstm_grad_part_floats(H);
    g.count = count; g.num_tiles = tiles; g.W = W; g.out_act = out_activation;
    head_grads_into(g, *grads);
    hipLaunchKernelGGL(fe_lstm_grad_pack_kernel, dim3(grid_for(lstm_grad_wt_floats(H))), dim3(kBlock), 0, (hipStream_t)stream,
                       g, H);
    if (int rc = launched("fe_lstm_backward: weight transpose")) return rc;
    const void *kern = with_nt(H, [](auto NT) { return (const void *)fe_lstm_grad_kernel<decltype(NT)::value>; });
    if (int rc = launch_grad(env, kern, lds, max_groups, 1, &g, &g.groups,
                             "LSTM head gradient kernel: hipFuncSetAttribute / occupancy query", "fe_lstm_backward: backward",
                             stream))
        return rc;
    hipLaunchKernelGGL(fe_lstm_grad_reduce_kernel, dim3(grid_for(lstm_grad_part_floats(H))), dim3(kBlock), 0,
                       (hipStream_t)stream, g, H);
    return launched("fe_lstm_backward: reduction");
}


// ---- include/finenvs_amd_lstm_grad_streamed.h: the one-output LSTM head's backward pass at H = 256 / 512 / 1024 ----
int64_t fe_lstm_streamed_grad_chunk_pairs(int32_t H, int32_t W) {
    if (!lstm_sgrad_hidden_ok(H) || W < 1) return -1;
    return lstm_sgrad_chunk_pairs(H, W);
}

// Workspace: [W_hh^T][split sums][head block sums][gates][c][h_{t-1} | x_t | 1][h_W][dh][dc], the last six for the pairs
// of one pass.
int64_t fe_lstm_streamed_grad_workspace_floats(int32_t H, int32_t W, int64_t count) {
    if (!lstm_sgrad_hidden_ok(H) || W < 1 || count < 0) return -1;
    const int64_t pp = lstm_sgrad_padded_pairs(H, W, count);
    return lstm_sgrad_wt_floats(H) + lstm_sgrad_splits(H, W, pp) * lstm_sgrad_part_floats(H) +
           lstm_sgrad_head_blocks(pp) * (H + 32) + pp * (lstm_sgrad_pair_floats(H, W) + 3LL * H);
}

// The recurrence kernel of the streamed head's and the streamed SAC actor's backward pass.
static const void *lstm_sgrad_forward_kernel_for(int32_t H) {
    return with_nt<64, 4>(H, [](auto NT) { return (const void *)fe_lstm_sgrad_forward_kernel<decltype(NT)::value>; });
}

// (declared with launch_twin_q_streamed; here for the order of the instantiations)
static const void *critic_sgrad_kernel(int32_t H, bool stash) {
    return !stash ? critic_sgrad_forward_kernel_for<false>(H) : critic_sgrad_forward_kernel_for<true>(H);
}

int fe_lstm_backward_streamed(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wout,
                              int32_t H, int32_t out_activation, const int64_t *obs_src, const double *obs_pos,
                              int64_t count, const float *outputs, const float *d_outputs, float *workspace,
                              const fe_lstm_grads *grads, void *stream) {
    static const char *who = "fe_lstm_backward_streamed";
    if (int rc = lstm_backward_checked(env, logret_f32, {whh, wx, wout, 0.0f, nullptr}, H, out_activation, obs_src, obs_pos,
                                       count, outputs, d_outputs, workspace, grads, true, who))
        return rc;
    if (count == 0) return FE_OK;
    const size_t lds = lstm_sgrad_forward_lds_bytes(H);
    if (int rc = lds_fits(lds, H, who)) return rc;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    const int W = env->p.W;
    hipStream_t st = (hipStream_t)stream;
    LstmSGradArgs g;
    memset(&g, 0, sizeof(g));
    g.lr32 = logret_f32; g.whh = whh; g.wx = wx; g.wout = wout; g.W = W; g.out_act = out_activation;
    sgrad_carve(g, workspace, H, lstm_sgrad_padded_pairs(H, W, count));
    head_grads_into(g, *grads);
    hipLaunchKernelGGL(fe_lstm_sgrad_pack_kernel, dim3(grid_for(lstm_sgrad_wt_floats(H))), dim3(kBlock), 0, st, g, H);
    if (int rc = launched("fe_lstm_backward_streamed: weight transpose")) return rc;
    return sgrad_chunks(env, who, g, H, count, obs_src, obs_pos, lstm_sgrad_forward_kernel_for(H), lds, &g,
                        "streamed LSTM head gradient kernel: hipFuncSetAttribute / occupancy query", nullptr,
                        fe_lstm_sgrad_final_kernel, nullptr, st, [&](int64_t c0) {
                            g.outputs = outputs ? outputs + c0 : nullptr;
                            g.d_outputs = d_outputs + c0;
                        });
}

// ---- include/finenvs_amd_sac.h and include/finenvs_amd_sac_streamed.h: the SAC actor's head on the LSTM recurrence,
// register-resident (launch_sac, above) and at H = 256 / 512 / 1024 ----
// Shared by fe_env_rollout_sac_streamed and fe_sac_forward_streamed: the fused form at every count (no split by time step).
static int launch_sac_streamed(fe_env *env, SacArgs &s, int64_t count, const char *who, void *stream) {
    const int32_t H = s.l.H;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    Params p = env->p;
    if (s.l.forward_only) p.eval_env = -1;
    const int SP = lstm_geometry(env, p, count, H, true, who);
    if (SP == 0) return FE_ERR_ARG;
    const size_t lds = sac_big_lds_bytes(p.EB, p.A, H);
    if (int rc = lds_fits(lds, H, who)) return rc;
    const void *kern = with_nt<64, 4>(p.A == 1, H, [](auto S, auto NT) { return (const void *)fe_rollout_sac_big_kernel<decltype(S)::value, decltype(NT)::value>; });
    return launch_resident(env, kern, lds, p, &s, "streamed SAC kernel", stream);
}

// The actor's part of a kernel's SacArgs.
static void sac_args(SacArgs &s, const float *logret_f32, const SacActorView &w, int32_t H) {
    s.bmu_p = w.bmu_p; s.bstd_p = w.bstd_p;
    s.l.lr32 = logret_f32; s.l.whh = w.whh; s.l.wx = w.wx; s.l.wout = nullptr; s.l.bout = 0.0f; s.l.H = H; s.l.out_act = 0;
    s.l.std = 0.0f;
    s.wl = w.wl; s.bl = w.bl; s.wmu = w.wmu; s.bmu = w.bmu; s.wstd = w.wstd; s.bstd = w.bstd;
}

// fe_env_rollout_sac, its _p sibling (both report as fe_env_rollout_sac) and fe_env_rollout_sac_streamed.  The resident
// entries refuse H in launch_sac, after the state is known to be bound.
static int rollout_sac_impl(fe_env *env, const float *logret_f32, const SacActorView &w, int32_t H, int32_t K, int64_t *obs_src,
                            double *obs_pos, const float *noise, float *actions_out, float *means_out, float *stds_out,
                            double *rewards_out, int32_t *dones_out, int64_t *states_src_out, double *states_pos_out,
                            void *stream, bool streamed, const char *who) {
    const bool given = env && logret_f32 && sac_view_given(w) && obs_src && obs_pos && rewards_out && dones_out && K >= 1;
    // unpaired descriptor outputs: the resident entries' first refusal, the streamed entry's second
    if ((states_src_out == nullptr) != (states_pos_out == nullptr) && (given || !streamed))
        return fail(FE_ERR_ARG, "%s: states_src_out and states_pos_out go together", who);
    if (!given) return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (streamed) {
        if (int rc = sac_streamed_hidden(H, who, "fe_env_rollout_sac")) return rc;
    }
    if (int rc = require_bound(env, who)) return rc;
    SacArgs s;
    sac_args(s, logret_f32, w, H);
    s.l.K = K; s.l.obs_src = obs_src; s.l.obs_pos = obs_pos; s.l.noise = noise; s.l.actions_out = actions_out;
    s.l.means_out = means_out; s.l.rew_out = rewards_out; s.l.done_out = dones_out; s.l.traj_src = states_src_out;
    s.l.traj_pos = states_pos_out; s.l.forward_only = 0;
    s.stds_out = stds_out; s.logp_out = nullptr;
    return streamed ? launch_sac_streamed(env, s, env->cfg.N, who, stream) : launch_sac(env, s, env->cfg.N, who, stream);
}

// fe_sac_forward, its _p sibling (both report as fe_sac_forward) and fe_sac_forward_streamed.  The resident entries
// refuse H in launch_sac, after count == 0 has returned.
static int sac_forward_impl(fe_env *env, const float *logret_f32, const SacActorView &w, int32_t H, const int64_t *obs_src,
                            const double *obs_pos, int64_t count, const float *noise, float *actions_out,
                            float *log_probs_out, float *means_out, float *stds_out, void *stream, bool streamed,
                            const char *who) {
    if (!env || !logret_f32 || !sac_view_given(w) || !obs_src || !obs_pos || count < 0)
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (!noise && (actions_out || log_probs_out))
        return fail(FE_ERR_ARG, "%s: actions_out and log_probs_out need noise", who);
    if (streamed) {
        if (int rc = sac_streamed_hidden(H, who, "fe_sac_forward")) return rc;
    }
    if (count == 0) return FE_OK;
    SacArgs s;
    sac_args(s, logret_f32, w, H);
    s.l.K = 1;
    s.l.obs_src = const_cast<int64_t *>(obs_src); s.l.obs_pos = const_cast<double *>(obs_pos);  // read only in this mode
    s.l.noise = noise; s.l.actions_out = actions_out; s.l.means_out = means_out; s.l.rew_out = nullptr; s.l.done_out = nullptr;
    s.l.traj_src = nullptr; s.l.traj_pos = nullptr; s.l.forward_only = 1;
    s.stds_out = stds_out; s.logp_out = log_probs_out;
    return streamed ? launch_sac_streamed(env, s, count, who, stream) : launch_sac(env, s, count, who, stream);
}

int fe_env_rollout_sac(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                       const float *bl, const float *wmu, float bmu, const float *wstd, float bstd, int32_t H, int32_t K,
                       int64_t *obs_src, double *obs_pos, const float *noise, float *actions_out, float *means_out,
                       float *stds_out, double *rewards_out, int32_t *dones_out, int64_t *states_src_out,
                       double *states_pos_out, void *stream) {
    return rollout_sac_impl(env, logret_f32, {whh, wx, wl, bl, wmu, wstd, bmu, bstd, nullptr, nullptr}, H, K, obs_src, obs_pos,
                            noise, actions_out, means_out, stds_out, rewards_out, dones_out, states_src_out, states_pos_out,
                            stream, false, "fe_env_rollout_sac");
}

int fe_env_rollout_sac_streamed(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                                const float *bl, const float *wmu, const float *bmu, const float *wstd, const float *bstd,
                                int32_t H, int32_t K, int64_t *obs_src, double *obs_pos, const float *noise,
                                float *actions_out, float *means_out, float *stds_out, double *rewards_out,
                                int32_t *dones_out, int64_t *states_src_out, double *states_pos_out, void *stream) {
    if (!bmu || !bstd) return fail(FE_ERR_ARG, "fe_env_rollout_sac_streamed: bad argument");
    return rollout_sac_impl(env, logret_f32, {whh, wx, wl, bl, wmu, wstd, 0.0f, 0.0f, bmu, bstd}, H, K, obs_src, obs_pos, noise,
                            actions_out, means_out, stds_out, rewards_out, dones_out, states_src_out, states_pos_out, stream,
                            true, "fe_env_rollout_sac_streamed");
}

int fe_sac_forward(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl, const float *bl,
                   const float *wmu, float bmu, const float *wstd, float bstd, int32_t H, const int64_t *obs_src,
                   const double *obs_pos, int64_t count, const float *noise, float *actions_out, float *log_probs_out,
                   float *means_out, float *stds_out, void *stream) {
    return sac_forward_impl(env, logret_f32, {whh, wx, wl, bl, wmu, wstd, bmu, bstd, nullptr, nullptr}, H, obs_src, obs_pos,
                            count, noise, actions_out, log_probs_out, means_out, stds_out, stream, false, "fe_sac_forward");
}

int fe_sac_forward_streamed(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                            const float *bl, const float *wmu, const float *bmu, const float *wstd, const float *bstd,
                            int32_t H, const int64_t *obs_src, const double *obs_pos, int64_t count, const float *noise,
                            float *actions_out, float *log_probs_out, float *means_out, float *stds_out, void *stream) {
    if (!bmu || !bstd) return fail(FE_ERR_ARG, "fe_sac_forward_streamed: bad argument");
    return sac_forward_impl(env, logret_f32, {whh, wx, wl, bl, wmu, wstd, 0.0f, 0.0f, bmu, bstd}, H, obs_src, obs_pos, count,
                            noise, actions_out, log_probs_out, means_out, stds_out, stream, true, "fe_sac_forward_streamed");
}

// Workspace: [W_l^T][split sums of d W_l][head block sums][z][the head's dz], sized by the largest pass, then the workspace
// of fe_lstm_backward_streamed.
int64_t fe_sac_streamed_grad_workspace_floats(int32_t H, int32_t W, int64_t count) {
    if (!lstm_sgrad_hidden_ok(H) || W < 1 || count < 0) return -1;
    return sac_sgrad_extra_floats(H, lstm_sgrad_padded_pairs(H, W, count)) + fe_lstm_streamed_grad_workspace_floats(H, W, count);
}

int fe_sac_backward_streamed(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                             const float *bl, const float *wmu, const float *bmu, const float *wstd, const float *bstd,
                             int32_t H, const int64_t *obs_src, const double *obs_pos, int64_t count, const float *noise,
                             const float *actions, const float *stds, const float *d_actions, const float *d_log_probs,
                             float *workspace, const fe_sac_grads *grads, void *stream) {
    static const char *who = "fe_sac_backward_streamed";
    if (!bmu || !bstd) return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (int rc = sac_backward_checked(env, logret_f32, {whh, wx, wl, bl, wmu, wstd, 0.0f, 0.0f, bmu, bstd}, H, obs_src, obs_pos,
                                      count, noise, actions, stds, d_actions, d_log_probs, workspace, grads, true, who))
        return rc;
    if (count == 0) return FE_OK;
    const size_t lds = lstm_sgrad_forward_lds_bytes(H);
    if (int rc = lds_fits(lds, H, who)) return rc;
    DeviceGuard guard(env->device);
    if (int rc = guard.status()) return rc;
    const int W = env->p.W;
    const int64_t pp = lstm_sgrad_padded_pairs(H, W, count);
    hipStream_t st = (hipStream_t)stream;
    SacSGradArgs a;
    memset(&a, 0, sizeof(a));
    LstmSGradArgs &g = a.g;
    g.lr32 = logret_f32; g.whh = whh; g.wx = wx; g.W = W;
    a.wl = wl; a.bl = bl; a.wmu = wmu; a.wstd = wstd; a.bstd = bstd;
    a.wlt = workspace;
    a.lpart = a.wlt + (int64_t)H * H;
    a.hpart2 = a.lpart + sac_sgrad_wl_splits(H, pp) * (int64_t)H * H;
    a.z = a.hpart2 + lstm_sgrad_head_blocks(pp) * sac_sgrad_hpart_floats(H);
    a.dzh = a.z + pp * H;
    sgrad_carve(g, a.dzh + pp * H, H, pp);
    g.g_wih = grads->w_ih; g.g_whh = grads->w_hh; g.g_bih = grads->b_ih; g.g_bhh = grads->b_hh; g.g_wout = grads->w_mu;
    g.g_bout = grads->b_mu;
    a.g_wl = grads->w_l; a.g_bl = grads->b_l; a.g_wstd = grads->w_std; a.g_bstd = grads->b_std;
    hipLaunchKernelGGL(fe_lstm_sgrad_pack_kernel, dim3(grid_for(lstm_sgrad_wt_floats(H))), dim3(kBlock), 0, st, g, H);
    hipLaunchKernelGGL(fe_sac_sgrad_pack_kernel, dim3(grid_for((int64_t)H * H)), dim3(kBlock), 0, st, a, H);
    if (int rc = launched("fe_sac_backward_streamed: weight transposes")) return rc;
    // (the chunks are the head's)
    return sgrad_chunks(env, who, g, H, count, obs_src, obs_pos, lstm_sgrad_forward_kernel_for(H), lds, &g,
                        "streamed SAC gradient kernel: hipFuncSetAttribute / occupancy query", nullptr, nullptr, &a, st,
                        [&](int64_t c0) {
                            a.wl_splits = sac_sgrad_wl_splits(H, g.pp);
                            a.noise = noise + c0; a.actions = actions + c0; a.stds = stds + c0;
                            a.d_actions = d_actions ? d_actions + c0 : nullptr;
                            a.d_log_probs = d_log_probs ? d_log_probs + c0 : nullptr;
                        });
}

// ---- include/finenvs_amd_optim.h: the entries above with their output biases in device memory ----
int fe_lstm_forward_p(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wout,
                      const float *bout, int32_t H, int32_t out_activation, const int64_t *obs_src, const double *obs_pos,
                      int64_t count, float *out, void *stream) {
    if (!bout) return fail(FE_ERR_ARG, "fe_lstm_forward_p: bad argument");
    return lstm_forward_impl(env, logret_f32, {whh, wx, wout, 0.0f, bout}, H, out_activation, obs_src, obs_pos, count, out,
                             stream);
}

int fe_env_rollout_lstm_p(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wout,
                          const float *bout, int32_t H, int32_t out_activation, int32_t K, int64_t *obs_src,
                          double *obs_pos, const float *noise, float std, float *actions_out, float *means_out,
                          double *rewards_out, int32_t *dones_out, int64_t *states_src_out, double *states_pos_out,
                          void *stream) {
    if (!bout) return fail(FE_ERR_ARG, "fe_env_rollout_lstm_p: bad argument");
    return rollout_lstm_impl(env, logret_f32, {whh, wx, wout, 0.0f, bout}, H, out_activation, K, obs_src, obs_pos, noise, std,
                             actions_out, means_out, rewards_out, dones_out, states_src_out, states_pos_out, stream);
}

int fe_env_rollout_lstm_split_p(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wout,
                                const float *bout, int32_t H, int32_t out_activation, int32_t K, int64_t *obs_src,
                                double *obs_pos, const float *noise, float std, float *actions_out, float *means_out,
                                double *rewards_out, int32_t *dones_out, int64_t *states_src_out, double *states_pos_out,
                                float *workspace, void *stream) {
    if (!bout) return fail(FE_ERR_ARG, "fe_env_rollout_lstm_split_p: bad argument");
    return rollout_lstm_split_impl(env, logret_f32, {whh, wx, wout, 0.0f, bout}, H, out_activation, K, obs_src, obs_pos, noise,
                                   std, actions_out, means_out, rewards_out, dones_out, states_src_out, states_pos_out,
                                   workspace, stream);
}

int fe_env_rollout_sac_p(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                         const float *bl, const float *wmu, const float *bmu, const float *wstd, const float *bstd,
                         int32_t H, int32_t K, int64_t *obs_src, double *obs_pos, const float *noise, float *actions_out,
                         float *means_out, float *stds_out, double *rewards_out, int32_t *dones_out,
                         int64_t *states_src_out, double *states_pos_out, void *stream) {
    if (!bmu || !bstd) return fail(FE_ERR_ARG, "fe_env_rollout_sac_p: bad argument");
    return rollout_sac_impl(env, logret_f32, {whh, wx, wl, bl, wmu, wstd, 0.0f, 0.0f, bmu, bstd}, H, K, obs_src, obs_pos, noise,
                            actions_out, means_out, stds_out, rewards_out, dones_out, states_src_out, states_pos_out, stream,
                            false, "fe_env_rollout_sac");
}

int fe_sac_forward_p(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                     const float *bl, const float *wmu, const float *bmu, const float *wstd, const float *bstd, int32_t H,
                     const int64_t *obs_src, const double *obs_pos, int64_t count, const float *noise, float *actions_out,
                     float *log_probs_out, float *means_out, float *stds_out, void *stream) {
    if (!bmu || !bstd) return fail(FE_ERR_ARG, "fe_sac_forward_p: bad argument");
    return sac_forward_impl(env, logret_f32, {whh, wx, wl, bl, wmu, wstd, 0.0f, 0.0f, bmu, bstd}, H, obs_src, obs_pos, count,
                            noise, actions_out, log_probs_out, means_out, stds_out, stream, false, "fe_sac_forward");
}

int fe_sac_backward_p(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                      const float *bl, const float *wmu, const float *bmu, const float *wstd, const float *bstd, int32_t H,
                      const int64_t *obs_src, const double *obs_pos, int64_t count, const float *noise,
                      const float *actions, const float *stds, const float *d_actions, const float *d_log_probs,
                      float *workspace, const fe_sac_grads *grads, void *stream) {
    if (!bmu || !bstd) return fail(FE_ERR_ARG, "fe_sac_backward_p: bad argument");
    return sac_backward_impl(env, logret_f32, {whh, wx, wl, bl, wmu, wstd, 0.0f, 0.0f, bmu, bstd}, H, obs_src, obs_pos, count,
                             noise, actions, stds, d_actions, d_log_probs, workspace, grads, stream);
}

// ---- include/finenvs_amd_optim.h: Adam, the soft update and the packing of every registered network, one launch ----
int fe_net_update(const fe_optim_desc *desc, void *stream) {
    if (!desc || !desc->segments || !desc->state || desc->num_segments < 1 || desc->num_blocks < 1 ||
        desc->num_blocks > 0x7fffffffll)
        return fail(FE_ERR_ARG, "fe_net_update: bad argument");
    if (desc->mode != FE_OPTIM_STEP && desc->mode != FE_OPTIM_PACK && desc->mode != FE_OPTIM_ZERO_GRAD)
        return fail(FE_ERR_ARG, "fe_net_update: mode must be FE_OPTIM_STEP, FE_OPTIM_PACK or FE_OPTIM_ZERO_GRAD (got %d)",
                    (int)desc->mode);
    if (desc->mode == FE_OPTIM_STEP &&
        !(desc->beta1 >= 0.0 && desc->beta1 < 1.0 && desc->beta2 >= 0.0 && desc->beta2 < 1.0 && desc->lr >= 0.0 &&
          desc->eps >= 0.0f))
        return fail(FE_ERR_ARG, "fe_net_update: lr and eps must be >= 0 and the betas in [0, 1)");
    DeviceGuard guard(device_of(desc->segments));
    if (int rc = guard.status("fe_net_update: the segment table is not device memory")) return rc;
    OptimArgs a;
    a.seg = desc->segments; a.st = desc->state; a.num_segments = desc->num_segments; a.mode = desc->mode;
    a.soft_update = desc->soft_update; a.zero_grad = desc->zero_grad;
    a.beta1 = desc->beta1; a.beta2 = desc->beta2; a.lr = desc->lr;
    a.omb1 = desc->one_minus_beta1; a.b2 = desc->beta2_f32; a.omb2 = desc->one_minus_beta2; a.eps = desc->eps;
    hipLaunchKernelGGL(fe_net_update_kernel, dim3((unsigned)desc->num_blocks), dim3(kBlock), 0, (hipStream_t)stream, a);
    return launched("fe_net_update");
}


// ---- include/finenvs_amd_ppo.h: PPO's mini-batch, epoch counter and losses ----
int fe_ppo_minibatch(const int64_t *obs_src, const double *obs_pos, const float *actions, int64_t T, int64_t N,
                     int64_t C, int32_t A, const float *const *columns, float *const *columns_out, int32_t num_columns,
                     int64_t *cursor, uint64_t seed, int64_t epoch_offset, int64_t M, int64_t m, int64_t *indices_out,
                     int64_t *obs_src_out, double *obs_pos_out, float *actions_out, void *stream) {
    if (!obs_src || !obs_pos || !actions || !cursor || !indices_out)
        return fail(FE_ERR_ARG, "fe_ppo_minibatch: null trajectory, cursor or indices_out");
    if (T < 1 || N < 1 || C < N || A < 1) return fail(FE_ERR_ARG, "fe_ppo_minibatch: need T >= 1, N >= 1, C >= N, A >= 1");
    const int64_t lim = (int64_t)1 << 32;
    if (T >= lim || N >= lim || T * N >= lim)
        return fail(FE_ERR_ARG, "fe_ppo_minibatch: T * N = %lld x %lld samples do not fit the 32-bit permutation",
                    (long long)T, (long long)N);
    const int64_t n = T * N;
    if (M < 1 || M > n || m < 0 || m >= M)
        return fail(FE_ERR_ARG, "fe_ppo_minibatch: mini-batch %lld of %lld over %lld samples", (long long)m, (long long)M, (long long)n);
    if (epoch_offset < 0) return fail(FE_ERR_ARG, "fe_ppo_minibatch: epoch_offset < 0");
    if (num_columns < 0 || num_columns > FE_PPO_MAX_COLUMNS || (num_columns > 0 && !columns))
        return fail(FE_ERR_ARG, "fe_ppo_minibatch: at most %d columns", FE_PPO_MAX_COLUMNS);
    for (int c = 0; c < num_columns; ++c)
        if (!columns[c]) return fail(FE_ERR_ARG, "fe_ppo_minibatch: column %d is null", c);
    DeviceGuard guard(device_of(obs_src));
    if (int rc = guard.status("fe_ppo_minibatch: the trajectory is not device memory")) return rc;
    PpoMinibatchArgs d;
    d.obs_src = obs_src; d.obs_pos = obs_pos; d.actions = actions;
    for (int c = 0; c < kPpoMaxColumns; ++c) {
        d.col[c] = c < num_columns ? columns[c] : nullptr;
        d.col_out[c] = c < num_columns && columns_out ? columns_out[c] : nullptr;
    }
    d.cursor = cursor; d.key = seed ^ FE_PPO_PERM_SALT; d.epoch_offset = epoch_offset;
    d.T = T; d.N = N; d.C = C; d.n = n; d.B = n / M; d.first = m * d.B; d.A = A;
    int k = 0;  // bit_length(n - 1)
    while (k < 32 && ((uint64_t)(n - 1) >> k) != 0) ++k;
    if (k < 1) k = 1;
    d.hb = (k + 1) / 2;
    d.idx = indices_out; d.src_out = obs_src_out; d.pos_out = obs_pos_out; d.act_out = actions_out;
    hipLaunchKernelGGL(fe_ppo_minibatch_kernel, dim3(grid_for(d.B * A)), dim3(kBlock), 0, (hipStream_t)stream, d);
    return launched("fe_ppo_minibatch");
}

int fe_ppo_epochs_advance(int64_t *cursor, int64_t count, void *stream) {
    if (!cursor || count < 0) return fail(FE_ERR_ARG, "fe_ppo_epochs_advance: bad argument");
    DeviceGuard guard(device_of(cursor));
    if (int rc = guard.status("fe_ppo_epochs_advance: the cursor is not device memory")) return rc;
    hipLaunchKernelGGL(fe_ppo_epochs_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, cursor, count);
    return launched("fe_ppo_epochs_advance");
}

static int ppo_loss_grid(int64_t count) {
    const int64_t g = (count + kBlock - 1) / kBlock;
    return (int)(g < kPpoLossMaxGrid ? g : kPpoLossMaxGrid);
}

int64_t fe_ppo_loss_workspace_doubles(int64_t count) {
    if (count < 1) return -1;
    return 1 + 2 * (int64_t)ppo_loss_grid(count);
}

int fe_ppo_actor_loss(const float *means, const float *log_std, const float *actions, const float *old_log_probs,
                      const float *advantages, int64_t count, double clip_epsilon, double entropy_coefficient,
                      float *loss, float *g_means, float *g_log_std, double *workspace, void *stream) {
    if (!means || !log_std || !actions || !old_log_probs || !advantages || !loss || !g_means || !g_log_std || !workspace ||
        count < 1 || !(clip_epsilon >= 0.0))
        return fail(FE_ERR_ARG, "fe_ppo_actor_loss: bad argument");
    DeviceGuard guard(device_of(means));
    if (int rc = guard.status("fe_ppo_actor_loss: means is not device memory")) return rc;
    PpoLossArgs d{};
    d.x = means; d.log_std = log_std; d.actions = actions; d.old_lp = old_log_probs; d.y = advantages; d.count = count;
    d.lo = 1.0 - clip_epsilon; d.hi = 1.0 + clip_epsilon; d.ent_coef = entropy_coefficient;
    d.loss = loss; d.g_x = g_means; d.g_log_std = g_log_std; d.ws = workspace;
    hipLaunchKernelGGL(fe_ppo_actor_loss_kernel, dim3(ppo_loss_grid(count)), dim3(kBlock), 0, (hipStream_t)stream, d);
    return launched("fe_ppo_actor_loss");
}

int fe_ppo_value_loss(const float *values, const float *returns, int64_t count, float *loss, float *g_values,
                      double *workspace, void *stream) {
    if (!values || !returns || !loss || !g_values || !workspace || count < 1)
        return fail(FE_ERR_ARG, "fe_ppo_value_loss: bad argument");
    DeviceGuard guard(device_of(values));
    if (int rc = guard.status("fe_ppo_value_loss: values is not device memory")) return rc;
    PpoLossArgs d{};
    d.x = values; d.y = returns; d.count = count; d.loss = loss; d.g_x = g_values; d.ws = workspace;
    hipLaunchKernelGGL(fe_ppo_value_loss_kernel, dim3(ppo_loss_grid(count)), dim3(kBlock), 0, (hipStream_t)stream, d);
    return launched("fe_ppo_value_loss");
}

}  // extern "C"

// ---- what the library's other translation units (fe_mlp_critic.hip, fe_mlp_sac.hip, fe_evo.hip) need of this one: hidden visibility, as
// fe_set_error is shared with fe_csv.cpp.  Host code only: this unit's device code object is what it was. ----
// An env's window, asset count and device.
extern "C" __attribute__((visibility("hidden"))) void fe_env_shape_internal(const fe_env *env, int32_t *W, int32_t *A, int *device) {
    *W = env->p.W;
    *A = env->p.A;
    *device = env->device;
}

// Whether fe_env_bind_state has been called: fe_evo_rollout refuses an unbound env in words of its own.
extern "C" __attribute__((visibility("hidden"))) int fe_env_bound_internal(const fe_env *env) { return env->bound; }

// prepare_big_lds for a kernel of the other unit: one cache of (device, kernel) attributes for the whole library.
extern "C" __attribute__((visibility("hidden"))) int fe_prepare_big_lds_internal(int device, const void *kern, size_t lds,
                                                                                 const char *who) {
    return prepare_big_lds(device, kern, lds, who);
}

// What a K-step rollout of the third and fourth units (fe_mlp_sac.hip, fe_evo.hip) takes from the env, as rollout_mlp_sampled_impl does: the
// state is bound, a copy of the parameter block with the rollout's tile set (128 pairs per workgroup), and the grid.
extern "C" __attribute__((visibility("hidden"))) int fe_env_mlp_rollout_internal(const fe_env *env, const char *who, void *params_out,
                                                                                 size_t params_bytes, int64_t *grid_out) {
    if (int rc = require_bound(env, who)) return rc;
    if (params_bytes != sizeof(Params)) return fail(FE_ERR_STATE, "%s: the units disagree about the parameter block", who);
    Params p = env->p;
    *grid_out = rollout_geometry(env, p, mlp_tile_envs(p), /*replace=*/true);
    memcpy(params_out, &p, sizeof(p));
    return FE_OK;
}
