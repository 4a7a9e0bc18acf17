#pragma once
// qpolicy.h — the DQN policy step fused on MFMA: the
// network handle se_qnet with its packed weights (QnetDims), the policy kernels,
// policy_call with launch_policy / launch_policy_x3, and the se_qnet_* / se_policy_* entry points.
// The device side lies in fragments of its own, one stage each, included below in this order:
// qnet_image.h (the images' layouts), qnet_parts.h (what the DQN kernels share, qnet_rollout.h's
// and qtrain.h's included), qnet_pack.h (the packers), qnet_order.h (the visiting order),
// qnet_trace.h (diagnostic stamps), policy_bf16.h (policy_kernel) and policy_x3.h
// (policy_x3_kernel). This file holds the host side.
//
// A fragment of shipenv.hip's translation unit, included at its end after the host
// side: not a stand-alone header. Uses world.h (WorldDims, LdsWorld, stage_world,
// world_view), env_core.h (env_key), philox.h, and the host side's se_env,
// host.h (check_ready, fail, HIP_TRY, DeviceGuard, device_reserve, device_free, allow_lds,
// lds_bytes) and kBlock.
//
// Reference: agents/dqn.py DQNNetwork
// (:21-33: fc1 6+4P -> 128, relu, fc2 128 -> 128, relu, fc3 128 -> A = 4+P+250)
// and choose_action (:177-203), on preprocess_state rows (utils/preprocessing.py:25-62).
//
// Shape of the work: per env ~50 K MACs (fc2 + fc3) against 16 bytes of state, so
// the step is MFMA-bound, not HBM-bound. One wave takes 32 envs at a time with
// the batch on the MFMA's column (N) dimension: every layer is D = W·X with the
// weights W as the A operand (bf16 fragments pre-permuted into LDS, lane-linear,
// one ds_read_b128 per MFMA) and the activations X as the B operand in registers.
// A v_mfma_f32_32x32x16_bf16 result keeps the env on the lane and the feature rows
// in its 16 registers, so relu + bf16 packing of registers 8s..8s+7 is directly
// the next layer's k-step s (cdna_hip_programming.md §3, "accumulator tile as the
// next MFMA's operand"); the weights are stored in that step's permuted k order.
// fc1 has 6 live inputs (the port block is constant: folded into the bias) and
// runs as one k-step per row tile, with fuel split into bf16 hi + lo parts. Biases
// are the accumulators' initial values (f32). fc3's epilogue is the masked
// argmax: each lane keeps the first maximum over the valid rows it holds, and the
// two lane halves that share an env merge with one shuffle. Q never reaches HBM.
//
// fc3 runs over the compact row layout (QnetDims): only the actions some env can
// ever take, so at P = 5 two 32-row tiles where the full layout has three with a valid
// row (of nine); the full layout serves q_out (every row's Q, for tests / inspection).
//
// LDS: the packed network (113 KB at P = 5) plus the world image, one 1024-thread
// workgroup (16 waves, 4 per SIMD, <= 128 VGPRs) per CU for the whole launch. It fits
// 128 VGPRs with no spills and no scratch: check (-Rpass-analysis=kernel-resource-usage)
// after any edit that adds register pressure.

namespace {

#include "qnet_image.h"   // QnetDims, QnetX3Dims, the fragment element maps
#include "qnet_parts.h"   // what the DQN kernels share: split3, EnvValid, the argmax, choose_store, khalf_x3
#include "qnet_pack.h"    // qnet_pack_kernel, pack_x3_items, qnet_pack_x3_kernel
#include "qnet_order.h"   // OrderRun: the visiting order
#include "qnet_trace.h"   // SHIPENV_X3_TRACE stamps
#include "policy_bf16.h"  // policy_kernel
#include "policy_x3.h"    // policy_x3_kernel

}  // namespace

struct se_qnet {
    se_env* env = nullptr;  // must outlive the qnet (destroy the qnet first)
    int device = 0;
    int cus = 256;  // the device's compute units (se_qnet_create): the policy kernels' resident workgroups
    QnetDims q{}, qc{};  // the full layout (q_out) and the compact one, whose image follows
    const float* w[6] = {};  // the device weights of the last se_qnet_set_weights (se_qnet_repack)
    size_t c_off = 0;    // byte offset of the compact image
    uint8_t* d_img = nullptr;
    size_t img_bytes = 0;
    uint64_t world_version = 0;
    bool packed = false;
    uint8_t* d_img32 = nullptr;  // se_policy_f32's split image (the full layout's fc3, global)
    size_t img32_bytes = 0;
    // the visiting order's scratch list (order_chunk): used when n >= order_min_envs, resolved once
    // by se_qnet_create (SHIPENV_POLICY_ORDER: 0 never, 1 always; unset: from 2^16 envs; 2 always,
    // with the bf16 kernel's list in this global scratch as when it does not fit the LDS, which
    // otherwise happens only past ~10M envs)
    uint32_t* d_order = nullptr;
    size_t order_bytes = 0;
    int64_t order_min_envs = (int64_t)1 << 16;
    bool order_lds = true;
};

namespace {

// the bf16 images of both layouts from the weights w (one launch); bump: se_qnet_repack's counter
int launch_pack(se_qnet* qn, const float* const (&w)[6], int32_t* bump, void* stream) {
    const se_env* env = qn->env;
    PackArgs A{w[0], w[1], w[2], w[3], w[4], w[5], env->d_world, env->dims, {qn->q, qn->qc},
               {qn->d_img, qn->d_img + qn->c_off}, bump};
    qnet_pack_kernel<<<dim3(64, 2), 256, 0, (hipStream_t)stream>>>(A);
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

// Is the handle ready to play: it exists, its env is bound (bound: asked of the env too), its
// images are packed, and no port changed since (stale: the caller's words for that)
int qnet_ready(se_qnet* qn, bool bound = true,
               const char* stale = "ports changed since se_qnet_set_weights (the port block is folded into fc1)") {
    if (!qn) return fail(SE_EINVAL, "null qnet");
    if (bound) {
        const int rc = check_ready(qn->env);
        if (rc) return rc;
    }
    if (!qn->packed) return fail(SE_ESTATE, "se_qnet_set_weights has not been called");
    if (qn->world_version != qn->env->world_version) return fail(SE_ESTATE, stale);
    return SE_OK;
}

// Workgroups for n envs in 32-env tiles, `waves` tiles a workgroup at a time: one per share of
// the tiles, or the `resident` that the device holds at once, whose waves then stride over the tiles
int resident_grid(int64_t n, int waves, int64_t resident) {
    const int64_t tiles = (n + 31) / 32;
    const int64_t want = (tiles + waves - 1) / waves;
    return (int)(want < resident ? want : resident);
}

}  // namespace

extern "C" {

int se_qnet_create(se_qnet** out, se_env* env) {
    if (!out) return fail(SE_EINVAL, "null out");
    *out = nullptr;
    int rc = check_ready(env);
    if (rc) return rc;
    se_qnet* qn = new se_qnet;
    qn->env = env;
    qn->device = env->device;
    if (hipDeviceGetAttribute(&qn->cus, hipDeviceAttributeMultiprocessorCount, env->device) != hipSuccess)
        qn->cus = 256;
    if (const char* v = getenv("SHIPENV_POLICY_ORDER")) {
        qn->order_min_envs = atoi(v) != 0 ? 0 : INT64_MAX;
        qn->order_lds = atoi(v) != 2;
    }
    *out = qn;
    return SE_OK;
}

int se_qnet_set_weights(se_qnet* qn, const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* w3, const float* b3, void* stream) {
    if (!qn) return fail(SE_EINVAL, "null qnet");
    if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3) return fail(SE_EINVAL, "null weight pointer");
    se_env* env = qn->env;
    // SELECT validity is one uint64_t per port (SAME, sel): bit p is port p, so 64 ports at most
    if (env->dims.P < 1 || env->dims.P > 64) return fail(SE_EINVAL, "the fused policy supports 1..64 ports");
    DeviceGuard g(env->device);
    const QnetDims q = qnet_dims(env->dims.P);
    const QnetDims qc = qnet_dims(env->dims.P, true, env->cmax, env->fmax);
    const size_t c_off = ((size_t)q.bytes() + 255) & ~(size_t)255;
    int rc = device_reserve(qn->d_img, qn->img_bytes, c_off + (size_t)qc.bytes());
    if (rc) return rc;
    qn->q = q;
    qn->qc = qc;
    qn->c_off = c_off;
    const float* wp[6] = {w1, b1, w2, b2, w3, b3};
    rc = launch_pack(qn, wp, nullptr, stream);
    if (rc) return rc;
    for (int i = 0; i < 6; ++i) qn->w[i] = wp[i];
    qn->world_version = env->world_version;
    qn->packed = true;
    return SE_OK;
}

}  // extern "C"

namespace {
// the visiting order's chunk per workgroup (a multiple of 32) and the grid that covers n with
// it, and the scratch list (A.order, A.chunk); position order below order_min_envs
int policy_order(se_qnet* qn, int* grid, PolicyArgs& A) {
    se_env* env = qn->env;
    if (env->n < qn->order_min_envs) return SE_OK;
    const int64_t per = (env->n + *grid - 1) / *grid;
    const int64_t chunk = (per + 31) & ~(int64_t)31;
    const int64_t g = (env->n + chunk - 1) / chunk;
    const int rc = device_reserve(qn->d_order, qn->order_bytes, (size_t)(g * chunk) * sizeof(uint32_t));
    if (rc) return rc;
    *grid = (int)g;
    A.order = qn->d_order;
    A.chunk = chunk;
    return SE_OK;
}

struct PolicyRecord {
    uint32_t* pos;
    float* fuel;
    int32_t* act;
    int64_t head, cap;
};

// one policy call's arguments, as se_policy / se_policy_f32 take them, and the ring slots of
// se_policy_record (null: no record)
struct PolicyCall {
    int32_t* actions;
    double epsilon;
    uint32_t t;
    float* q_out;
    int64_t ldq;
    const PolicyRecord* rec;
    void* stream;
};

// What the two datapaths' launches share: everything but the visiting order (policy_order) and
// lds_list. q is the layout of the image at img.
PolicyArgs policy_args(const se_qnet* qn, const QnetDims& q, const uint8_t* img, const PolicyCall& c) {
    const se_env* env = qn->env;
    PolicyArgs A{};
    A.world = env->d_world;
    A.dims = env->dims;
    A.qimg = reinterpret_cast<const uint4*>(img);
    A.q = q;
    A.n = env->n;
    A.env_base = env->env_base;
    A.seed = env->seed;
    A.t = c.t;
    A.eps = c.epsilon;
    A.st = env->st;
    A.actions = c.actions;
    A.q_out = c.q_out;
    A.ldq = c.ldq;
    if (c.rec) {
        A.rec_pos = c.rec->pos;
        A.rec_fuel = c.rec->fuel;
        A.rec_act = c.rec->act;
        A.rec_head = c.rec->head;
        A.rec_cap = c.rec->cap;
    }
    return A;
}

// the bf16 datapath (policy_kernel); policy_call checked the arguments
int launch_policy(se_qnet* qn, const PolicyCall& c) {
    se_env* env = qn->env;
    // the compact layout unless every row's Q is wanted
    const QnetDims& q = c.q_out ? qn->q : qn->qc;
    size_t lds = (((size_t)q.bytes() + lds_bytes(env) + 7) & ~(size_t)7) + kOrderScanBytes;
    int rc = allow_lds<policy_kernel<false>>(kLdsMax, env->device);
    if (!rc) rc = allow_lds<policy_kernel<true>>(kLdsMax, env->device);
    if (rc) return rc;
    if (lds > kLdsMax) return fail(SE_EINVAL, "network + world image exceed the 160 KB LDS");
    int grid = resident_grid(env->n, kPolicyWaves, (int64_t)qn->cus * kPolicyWgPerCu);
    PolicyArgs A = policy_args(qn, q, qn->d_img + (c.q_out ? 0 : qn->c_off), c);
    rc = policy_order(qn, &grid, A);
    if (rc) return rc;
    A.lds_list = -1;
    if (A.order && qn->order_lds && A.chunk <= 0xffff && lds + (size_t)A.chunk * 2 <= kLdsMax) {  // the list in LDS
        A.lds_list = (int32_t)lds;
        lds += (size_t)A.chunk * 2;
    }
    if (c.q_out) {
        policy_kernel<true><<<grid, kPolicyBlock, lds, (hipStream_t)c.stream>>>(A);
    } else {
        policy_kernel<false><<<grid, kPolicyBlock, lds, (hipStream_t)c.stream>>>(A);
    }
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

// the split-bf16 datapath (policy_x3_kernel); policy_call checked the arguments
int launch_policy_x3(se_qnet* qn, const PolicyCall& c) {
    se_env* env = qn->env;
    QnetX3Dims d;
    d.q = c.q_out ? qn->q : qn->qc;  // the compact rows unless every row's Q is wanted
    // a zero row of fc3's last tile (row 32 mt3 - 1, past the layout's rows), or none
    d.zrow = d.q.rows < 32 * d.q.mt3 ? (d.q.mt3 - 1) * 8 * 192 + 31 : -1;
    int rc = device_reserve(qn->d_img32, qn->img32_bytes, (size_t)d.bytes());
    if (rc) return rc;
    const hipStream_t s = (hipStream_t)c.stream;
    // the image from the current weights (in place updates by an optimizer or T2 included)
    PackX3Args pk{qn->w[0], qn->w[1], qn->w[2], qn->w[3], qn->w[4], qn->w[5], env->d_world, env->dims, d,
                  qn->d_img32};
    constexpr int kPtabBytes = kX3PtabBytes;
    const bool w3_global = (size_t)(d.bytes() + kPtabBytes + kOrderScanBytes) > kLdsMax;
    if (w3_global) {  // fc3's fragments are read from a packed global image
        qnet_pack_x3_kernel<<<128, 256, 0, s>>>(pk);
        HIP_TRY(hipGetLastError());
    }
    const size_t lds = (size_t)(w3_global ? ((d.w3() + 7) & ~7) : ((d.bytes() + 15) & ~15) + kPtabBytes) +
                       kOrderScanBytes;
    if (lds > kLdsMax) return fail(SE_EINVAL, "split-bf16 network exceeds the 160 KB LDS");
    rc = allow_lds<policy_x3_kernel<false>>(kLdsMax, env->device);
    if (!rc) rc = allow_lds<policy_x3_kernel<true>>(kLdsMax, env->device);
    if (!rc) rc = allow_lds<policy_x3_kernel<true, true>>(kLdsMax, env->device);
    if (rc) return rc;
    int grid = resident_grid(env->n, kPolicyX3Waves, qn->cus);
    PolicyArgs A = policy_args(qn, d.q, qn->d_img32, c);
    rc = policy_order(qn, &grid, A);
    if (rc) return rc;
    if (c.q_out) {  // the full layout (fc3 from global memory): unmasked Q rows for q_out
        if (!w3_global) return fail(SE_EINVAL, "q_out: the full fc3 layout is expected in global memory");
        policy_x3_kernel<true, true><<<grid, kPolicyX3Block, lds, s>>>(A, d, pk);
    } else if (w3_global) {
        policy_x3_kernel<true><<<grid, kPolicyX3Block, lds, s>>>(A, d, pk);
    } else {
        policy_x3_kernel<false><<<grid, kPolicyX3Block, lds, s>>>(A, d, pk);
    }
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

// One policy call of either precision (launch: launch_policy or launch_policy_x3): the
// argument checks, in one order whatever the datapath, then the launch on the env's device.
int policy_call(int (*launch)(se_qnet*, const PolicyCall&), se_qnet* qn, const PolicyCall& c) {
    const int rc = qnet_ready(qn);
    if (rc) return rc;
    se_env* env = qn->env;
    if (!c.actions && env->n > 0) return fail(SE_EINVAL, "null actions");
    if (c.q_out && c.ldq < qn->q.A) return fail(SE_EINVAL, "ldq < number of actions");
    if (!(c.epsilon >= 0.0)) return fail(SE_EINVAL, "epsilon must be >= 0");
    if (env->n == 0) return SE_OK;
    DeviceGuard g(env->device);
    return launch(qn, c);
}

}  // namespace

extern "C" {

int se_policy(se_qnet* qn, int32_t* actions, double epsilon, uint32_t t, float* q_out, int64_t ldq,
              void* stream) {
    return policy_call(launch_policy, qn, {actions, epsilon, t, q_out, ldq, nullptr, stream});
}

int se_policy_f32(se_qnet* qn, int32_t* actions, double epsilon, uint32_t t, float* q_out, int64_t ldq,
                  void* stream) {
    return policy_call(launch_policy_x3, qn, {actions, epsilon, t, q_out, ldq, nullptr, stream});
}

#if SHIPENV_X3_TRACE
int se_policy_trace_read(void* host, size_t bytes) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_ptrace), bytes) == hipSuccess ? 0 : -1;
}
#endif

int se_qnet_repack(se_qnet* qn, int32_t* bump, void* stream) {
    // the env's binding is not asked about: as before, only the handle's own state
    const int rc = qnet_ready(qn, false, "ports changed: call se_qnet_set_weights (the port block is folded into fc1)");
    if (rc) return rc;
    DeviceGuard g(qn->env->device);
    return launch_pack(qn, qn->w, bump, stream);
}

int se_qnet_destroy(se_qnet* qn) {
    if (!qn) return SE_OK;
    if (qn->d_img || qn->d_img32 || qn->d_order) {  // does not touch the env, which may be gone already
        DeviceGuard g(qn->device);
        (void)hipDeviceSynchronize();
        (void)device_free({qn->d_img, qn->d_img32, qn->d_order});
    }
    delete qn;
    return SE_OK;
}

}  // extern "C"
