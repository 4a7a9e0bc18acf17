#pragma once
// qnet_rollout.h — network-policy rollouts (an extension: the reference values its DQN only by
// stepping the training envs): qnet_rollout_kernel, episode.h's scaffold around the MFMA policy
// and the step fused in one position loop, and se_rollout_qnet.
//
// A fragment of shipenv.hip's translation unit, included at its end after qpolicy.h: not a
// stand-alone header. Uses qpolicy.h (se_qnet, qnet_ready, resident_grid) and its fragments
// qnet_image.h (QnetDims and the packed compact image, the SAME table) and qnet_parts.h (split3,
// obs_frag, bias_frag, masked_bias, relu_pack, env_valid / tile_maybe / tile_mask,
// argmax_local_part, explore_choice), rollout.h (drawn_step), env_core.h (decode_agent),
// episode.h (EpisodeArgs,
// episode_lane, EpisodeTally, episode_store), philox.h and the host side's env_args, fail, HIP_TRY,
// DeviceGuard, allow_lds, lds_bytes and aligned16.
//
// The position is stated in include/shipenv.h. What it restates of the reference: choose_action
// (agents/dqn.py:177-203) exactly as policy_kernel does it for an env in the private ship's
// state, and the training loop's break on a raising step (:309-313). Position k draws what
// position k of every rollout kind draws, (k, slot 12) words 1-3 and (k, slot 13), so a network
// rollout equals se_rollout_plan (agent indices) of the actions it emitted. The explore block is
// (k, slot 22), drawn only where epsilon > 0: word 0 is the table rollout's explore uniform (the
// test here is se_policy's non-strict one), word 1 picks among the valid actions.
//
// Shape of the work: the MFMA's column is the env, so one wave owns a tile of 32 rollouts for the
// tile's whole life. Lanes l and l + 32 hold the same rollout: both carry the ship, the key and the
// tally and step them identically (the same draws, the same result), so nothing moves between
// lanes but the half-merge of the argmax; lane half 0 stores. The network image and the world are
// staged once per workgroup, as policy_kernel stages them, and stay in LDS for every position of
// every tile the workgroup plays.
//
// Registers: policy_kernel sits at the 128-VGPR limit of 16 waves per CU, and this kernel keeps
// the ship (f64 fuel), the key, the tally (an f64 and five ints) and the position live across the
// MFMA region on top of it. It therefore gives up the fourth wave per SIMD, as policy_x3_kernel
// does, and not the tally to LDS: it needs 146 VGPRs, which fits the 168 of 3 waves per SIMD, so
// the workgroup is 768 threads (512, 2 waves per SIMD, measured 12 % slower at 2^20 rollouts;
// DESIGN.md §9f has the figures). No scratch, no spills: check
// (-Rpass-analysis=kernel-resource-usage) after any edit that adds register pressure.
//
// Every Q row has se_policy's bits: the same fragments in the same k-step order, the biases as the
// accumulators' initial values, fc1's bias riding k = 8..10 in three bf16 parts, rows the ship
// cannot take at -inf (masked_bias; a valid row's chain is untouched by it), the same strict
// first maximum and the same half-merge. A fc3 tile no playing lane of the wave can choose from
// is skipped, MFMAs included; there is no visiting order (a tile's lanes are its rollouts for life).

namespace {

#ifndef SHIPENV_QROLL_BLOCK
#define SHIPENV_QROLL_BLOCK 768  // an A/B build may set 512 (2 waves per SIMD, a 256-VGPR budget)
#endif
constexpr int kQrollBlock = SHIPENV_QROLL_BLOCK;
constexpr int kQrollWaves = kQrollBlock / 64;

struct QrollArgs : EpisodeArgs {
    const uint4* qimg;  // the compact image of the last se_qnet_set_weights / se_qnet_repack
    QnetDims q;
    int32_t steps;
    double epsilon;
    se_qnet_out out;  // null pointers: not wanted
};

// The argument block read where it is used, through the kernarg segment (the kernel's one
// argument lies at its start): the tile's head and its stores read a dozen pointers that the
// position loop never touches, and as plain uses of the by-value argument they were loaded at
// the kernel's entry and spilled across the loop (72 SGPRs). The empty asm keeps the loads from
// being hoisted back.
__device__ __forceinline__ const QrollArgs& qroll_args_here() {
    auto p = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const QrollArgs*)p;
}

__global__ __launch_bounds__(kQrollBlock) void qnet_rollout_kernel(QrollArgs A) {
    extern __shared__ uint4 smem[];
    const QnetDims q = A.q;
    const int lane = threadIdx.x & 63, h = lane >> 5;
    // the image, fc1's bias in the padding half of its single k-step (policy_kernel's staging:
    // lanes 32-63 of each W1 fragment get the three bf16 parts of their row's b1), then the world
    const int qwords = q.bytes() / 16;
    const int w1w = q.w1() / 16, b1f = q.b1() / 4;
    for (int i = threadIdx.x; i < qwords; i += kQrollBlock) {
        const int k = i - w1w;  // W1 fragment (mt, lane) = k: mt = k >> 6, lane = k & 63
        if ((unsigned)k < 4u * 64u && (k & 32)) {
            const float b = reinterpret_cast<const float*>(A.qimg)[b1f + (k >> 6) * 32 + (k & 31)];
            __bf16 p0, p1, p2;
            split3(b, p0, p1, p2);
            bf16x8 v{};
            v[0] = p0;
            v[1] = p1;
            v[2] = p2;
            smem[i] = __builtin_bit_cast(uint4, v);
        } else {
            smem[i] = A.qimg[i];
        }
    }
    const LdsWorld w = stage_world(A.world, A.dims, reinterpret_cast<uint32_t*>(smem + qwords));
    const uint8_t* qb = reinterpret_cast<const uint8_t*>(smem);
    const bf16x8* W1f = reinterpret_cast<const bf16x8*>(qb + q.w1());
    const bf16x8* W2f = reinterpret_cast<const bf16x8*>(qb + q.w2());
    const bf16x8* W3f = reinterpret_cast<const bf16x8*>(qb + q.w3());
    const float* B2 = reinterpret_cast<const float*>(qb + q.b2());
    const float* B3 = reinterpret_cast<const float*>(qb + q.b3());
    const uint64_t* SAME = reinterpret_cast<const uint64_t*>(qb + q.same());
    const int P = q.P;
    const bool acts = A.out.act != nullptr;

    const int64_t tiles = (A.m + 31) >> 5;
    for (int64_t tile = (int64_t)blockIdx.x * kQrollWaves + (threadIdx.x >> 6); tile < tiles;
         tile += (int64_t)gridDim.x * kQrollWaves) {
        EpisodeLane L = episode_lane(qroll_args_here(), tile * 32 + (lane & 31));
        EpisodeTally T(L);
        int32_t explored = 0;
        bool alive = L.good & (A.steps > 0);
        int32_t k = 0;
#pragma nounroll
        for (; __ballot(alive) != 0ull; ++k) {
            // ---- choose_action on the private ship: every lane runs the network (the MFMA and
            // the half-merge are wave-wide); a lane that no longer plays computes on its last ship
            // and its column is dropped
            const int x = alive ? L.s.x : 0, y = alive ? L.s.y : 0;
            const int origin = L.s.origin == SE_NONE ? -1 : L.s.origin;
            const int dest = L.s.dest == SE_NONE ? -1 : L.s.dest;
            const float ff = (float)L.s.fuel;  // torch's .float() of the f64 fuel
            const bf16x8 ob = obs_frag(L.s.x, L.s.y, ff, origin, dest, h);
            bf16x8 h1[4][2], h2[4][2];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {  // fc1 + relu
                f32x16 c = {};
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W1f[mt * 64 + lane], ob, c, 0, 0, 0);
                relu_pack(c, h1[mt]);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {  // fc2 + relu, a row tile per pass
                bf16x8 wf[8];  // the tile's 8 fragments, read before the chain consumes them
#pragma unroll
                for (int s = 0; s < 8; ++s) wf[s] = W2f[(mt * 8 + s) * 64 + lane];
                f32x16 c = bias_frag(B2 + mt * 32 + 4 * h);
#pragma unroll
                for (int s = 0; s < 8; ++s)
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s], h1[s >> 1][s & 1], c, 0, 0, 0);
                relu_pack(c, h2[mt]);
            }
            // is_valid_action (dqn.py:125-175) of the ship, as row ranges of the compact layout
            const EnvValid v = env_valid(w, q, SAME, x, y, origin);
            float best = -INFINITY;
            int bidx = 0x7fffffff;
#pragma nounroll
            for (int mt = 0; mt < q.mt3; ++mt) {  // fc3 + the masked first-maximum argmax
                // a tile no playing lane of the wave can choose from is skipped, MFMAs included
                if (!__any(alive & tile_maybe(v, mt, P))) continue;
                bf16x8 wf[8];
#pragma unroll
                for (int s = 0; s < 8; ++s) wf[s] = W3f[(mt * 8 + s) * 64 + lane];
                f32x16 c = masked_bias(B3 + mt * 32 + 4 * h, tile_mask(v, mt, P) >> (4 * h));
#pragma unroll
                for (int s = 0; s < 8; ++s)
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s], h2[s >> 1][s & 1], c, 0, 0, 0);
                // ascending rows, strict >: the first maximum stays; the tile's base and the lane
                // half's rows are added once if the tile raised the maximum
                const float best0 = best;
                int bt = 0;
#pragma unroll
                for (int g = 0; g < 4; ++g) argmax_local_part(c, best, bt, g);
                bidx = best != best0 ? mt * 32 + 4 * h + bt : bidx;
            }
            // the two lane halves hold the same rollout: larger value, then lower index (both
            // halves end with the same winner; merge_halves, inline: the call moved this kernel's registers)
            const float ob2 = __shfl_xor(best, 32);
            const int oi = __shfl_xor(bidx, 32);
            if (ob2 > best || (ob2 == best && oi < bidx)) {
                best = ob2;
                bidx = oi;
            }
            int32_t emitted = SE_QROLL_PAD;
            if (alive) {
                // no valid action, or a fuel that is not finite (every Q is NaN then): 0 (:188-189)
                int act = ((bidx == 0x7fffffff) | !fuel_finite(ff)) ? 0 : q.action_of_row(bidx);
                if (A.epsilon > 0.0) {
                    const U4 e = draw(L.key, (uint32_t)k, kSlotRolloutQ);
                    if (u32(e.v[0]) <= A.epsilon) {  // np.random.rand() <= epsilon (:191)
                        act = explore_choice(v.sel, v.cst, v.fst, P, e.v[1]);
                        explored += 1;
                    }
                }
                // ---- the step, as se_rollout_plan steps position k of an agent-index plan
                const U4 d = draw(L.key, (uint32_t)k, kSlotRollout);
                int ty, va, vb;
                const int e_in = decode_agent(w.P, act, ty, va, vb);
                const Pending p = drawn_step(w, L.s, L.key, (uint32_t)k, kSlotRolloutB, d, ty, va, vb, e_in);
                T.add(p, k);
                // the training loop breaks on a raising step (dqn.py:309-313)
                T.status = p.e != SE_ERR_OK ? SE_PLAN_RAISED : T.status;
                alive = (p.e == SE_ERR_OK) & !T.done() & (k + 1 < A.steps);
                emitted = act;
            }
            if (acts & L.in & (h == 0)) A.out.act[(int64_t)k * A.out.ld + L.r] = emitted;
        }
        if (!L.in | (h != 0)) continue;
        if (acts) {
#pragma clang loop vectorize(disable) unroll(disable)
            for (; k < A.steps; ++k) A.out.act[(int64_t)k * A.out.ld + L.r] = SE_QROLL_PAD;
        }
        const QrollArgs& Z = qroll_args_here();
        episode_store(Z, Z.out.end, L, T);
        if (Z.out.explored) Z.out.explored[L.r] = explored;
    }
}

}  // namespace

extern "C" {

int se_rollout_qnet(se_qnet* qn, int32_t mode, double epsilon, const int32_t* src, int64_t m, const int64_t* ids,
                    int64_t rollout_base, int32_t steps, double* ret, int32_t* counted, int32_t* status,
                    const se_qnet_out* out, void* stream) {
    // the arguments first: misuse is reported whatever the handle's state
    if (m < 0 || steps < 0 || rollout_base < 0) return fail(SE_EINVAL, "m, steps and rollout_base must be >= 0");
    if (!(epsilon >= 0.0)) return fail(SE_EINVAL, "epsilon is NaN or negative");
    if (mode == 1) return fail(SE_EINVAL, "the fp32-faithful rollout is not built");
    if (mode != 0) return fail(SE_EINVAL, "unknown mode (0: bf16 as se_policy)");
    if (m > 0 && (!src || !ret || !counted || !status)) return fail(SE_EINVAL, "null rollout buffer");
    if (out && out->act) {
        if (out->ld < m) return fail(SE_EINVAL, "ld must be >= m");
        if (!aligned16(out->act) || (steps > 1 && (out->ld & 3)))
            return fail(SE_EINVAL, "action rows must be 16-byte aligned (row stride a multiple of 4)");
    }
    // then the handle, held to se_policy's readiness
    int rc = qnet_ready(qn);
    if (rc) return rc;
    se_env* env = qn->env;
    if (m == 0) return SE_OK;
    const QnetDims& q = qn->qc;  // the compact layout: only the actions some env can ever take
    const size_t lds = (size_t)q.bytes() + lds_bytes(env);
    if (lds > kLdsMax) return fail(SE_EINVAL, "network + world image exceed the 160 KB LDS");
    DeviceGuard g(env->device);
    rc = allow_lds<qnet_rollout_kernel>(kLdsMax, env->device);
    if (rc) return rc;
    QrollArgs A{};
    static_cast<EpisodeArgs&>(A) = {env_args(env), m, rollout_base, src, ids, ret, counted, status};
    A.qimg = reinterpret_cast<const uint4*>(qn->d_img + qn->c_off);
    A.q = q;
    A.steps = steps;
    A.epsilon = epsilon;
    if (out) A.out = *out;
    // one workgroup per CU stays resident; its waves take the tiles in a grid-stride loop
    const int grid = resident_grid(m, kQrollWaves, qn->cus);
    qnet_rollout_kernel<<<grid, kQrollBlock, lds, (hipStream_t)stream>>>(A);
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

}  // extern "C"
