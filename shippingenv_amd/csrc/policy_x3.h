#pragma once
// policy_x3.h — policy_x3_kernel, the split-bf16 f32 policy step (se_policy_f32).
//
// A fragment of shipenv.hip's translation unit, included inside qpolicy.h's anonymous
// namespace after its other fragments: not a stand-alone header. Uses qnet_image.h (QnetX3Dims,
// x3_fc1_slot), qnet_parts.h (PolicyArgs, EnvValid and its helpers, the argmax helpers,
// masked_bias, khalf_x3, x3_frags, split_pair, FINISH_ENV), qnet_pack.h (PackX3Args,
// pack_x3_items, kX3PtabBytes), qnet_order.h (OrderRun), qnet_trace.h (X3STAMP) and world.h
// (world_view, LdsWorld).
//
// ------------------------------------------------------------------ the split-bf16 f32 step
// The fp32-faithful form of the step (se_policy_f32): DQNNetwork evaluated as agents/dqn.py:198-200
// runs it (fp32 weights, fp32 activations), on bf16 MFMA (round 5; gfx950 has no xf32, and the
// round-4 form on v_mfma_f32_32x32x2_f32 took 0.43 ms per call at 2^20). fc1, fc2 and fc3 run
// on v_mfma_f32_32x32x16_bf16 with every f32 operand split into three bf16 parts,
// w = w0 + w1 + w2 and x = x0 + x1 + x2 (each part the round-to-nearest bf16 of what the
// parts before it leave; three 8-bit significands hold an f32's 24 bits), and the six
// products whose parts sum to at most 2, w0x2 + w1x1 + w2x0 + w0x1 + w1x0 + w0x0, smallest
// first, into one f32 accumulator. The dropped products (w1x2, w2x1, w2x2) are below
// 2^-23 of |w x|: a simulation of this datapath against float64 (MFMA = one f32 rounding
// per instruction) errs like the f32 MFMA path and torch's fp32 GEMM.
// Six bf16 MFMAs (32 cycles each) per 16-deep k-step where the f32 datapath runs eight
// v_mfma_f32_32x32x2_f32 (64 cycles each): 2.7x fewer MFMA cycles. fc1 (6 live inputs)
// runs as two split-bf16 MFMAs per row tile (x3_fc1_slot). Relu'd activations are split
// once per layer (registers 8s..8s+7 of tile kt are k-step (kt, s)'s B operand, as in the
// bf16 kernel) and held as 24 bf16x8 parts. Image: fc1 fragments, f32 biases, fc2 and fc3
// as three bf16 fragments per (tile, kt, s): 96 KB + 24 KB per fc3 tile, so the world is
// read in place (L2), not staged, and fc3 comes from global memory when it does not fit
// (the full layout). One 32-env tile per wave; 512-thread workgroups, one per CU.

constexpr int kPolicyX3Block = 512;

constexpr int kPolicyX3Waves = kPolicyX3Block / 64;

template <bool kW3Global, bool kQout = false>
__global__ __launch_bounds__(kPolicyX3Block) void policy_x3_kernel(PolicyArgs A, QnetX3Dims D, PackX3Args PK) {
    extern __shared__ uint4 smem[];
    X3STAMP_ANY(9);
    const QnetDims q = D.q;
    // the first tile's env state (an HBM round trip) is requested before the image is built,
    // so the two overlap
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int64_t tiles = (A.n + 31) >> 5;
    struct EnvIn {  // the four state bytes packed (x | y << 8 | origin << 16 | dest << 24): 2 VGPRs fewer
        double fuel;
        uint32_t pk;
        uint32_t e;  // the env (A.order), A.n for the last tile's idle lanes (n < 2^32: the order is u32)
        __device__ uint32_t x8() const { return pk & 0xffu; }
        __device__ uint32_t y8() const { return (pk >> 8) & 0xffu; }
        __device__ uint32_t o8() const { return (pk >> 16) & 0xffu; }
        __device__ uint32_t d8() const { return pk >> 24; }
    };
    // the visiting order: this workgroup's chunk and its list (null: position order)
    const uint32_t* ord = nullptr;
    int64_t c0 = 0;
    int len = 0;
    OrderRun orun;
    if (A.order) {  // loaded here, counted and placed once the image is built (the loads overlap it)
        c0 = (int64_t)blockIdx.x * A.chunk;
        len = __builtin_amdgcn_readfirstlane((int)min(A.chunk, A.n - c0));  // uniform: an SGPR
        orun.load<kPolicyX3Block>(A.st.x, A.st.y, c0, len);
    }
    auto load_env = [&](int64_t t) {
        const int64_t p = t * 32 + (lane & 31);
        int64_t ei;
        bool live;
        if (ord) {  // p < the chunk's whole tiles: its tail reads kOrderNone
            const uint32_t v = ord[p];
            live = v != kOrderNone;
            ei = live ? (int64_t)v : A.n - 1;
        } else {
            live = p < A.n;
            ei = live ? p : A.n - 1;
        }
        const uint32_t pk = (uint32_t)A.st.x[ei] | (uint32_t)A.st.y[ei] << 8 | (uint32_t)A.st.origin[ei] << 16 |
                            (uint32_t)A.st.dest[ei] << 24;
        return EnvIn{A.st.fuel[ei], pk, (uint32_t)(live ? ei : A.n)};
    };
    // tiles: the chunk's (waves round robin) or all of them (striding over the grid); in
    // position order the first tile's env state is requested before the image is built
    const bool ordered = A.order != nullptr;
    const int64_t my_tiles = ordered ? (len + 31) >> 5 : tiles;
    int64_t tile = ordered ? (threadIdx.x >> 6) : (int64_t)blockIdx.x * kPolicyX3Waves + (threadIdx.x >> 6);
    const int64_t stride = ordered ? kPolicyX3Waves : (int64_t)gridDim.x * kPolicyX3Waves;
    EnvIn nxt{};
    if (!ordered) nxt = load_env(tile < my_tiles ? tile : 0);
    if constexpr (kW3Global) {  // fc3 stays in the packed global image: copy the rest
        const int staged = D.w3() / 16;
        for (int i = threadIdx.x; i < staged; i += kPolicyX3Block) smem[i] = A.qimg[i];
    } else {
        // the whole image fits: each workgroup splits the f32 weights into its own LDS copy
        // (about 93 KB of f32 reads per workgroup at P = 5 where the packed image is 152 KB),
        // so no pack kernel runs before the policy and in-place weight updates are seen
        uint32_t* ptab = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(smem) + ((D.bytes() + 15) & ~15));
        {
            const LdsWorld wg = world_view(A.dims, A.world);
            const int t = threadIdx.x, P0 = A.dims.P;
            if (t < P0) ptab[t] = wg.pos[t];
            else if (t >= 64 && t < 64 + 2 * P0) ptab[t] = reinterpret_cast<const uint32_t*>(wg.stock)[t - 64];
        }
        __syncthreads();
        PackX3Args pk = PK;
        pk.ptab = ptab;
        pack_x3_items(pk, reinterpret_cast<uint8_t*>(smem), threadIdx.x, kPolicyX3Block);
    }
#if SHIPENV_X3_TRACE
    if ((threadIdx.x & 63) == 0)  // slot 15: the wave's part of the image built
        g_ptrace[(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) % 4096 * 16 + 15] = __builtin_amdgcn_s_memrealtime();
#endif
    __syncthreads();
    if (ordered) {
        uint32_t* list = A.order + c0;
        const int wo = kW3Global ? ((D.w3() + 7) & ~7) : (((D.bytes() + 15) & ~15) + kX3PtabBytes);
        const LdsWorld wg = world_view(A.dims, A.world);
        orun.count<kPolicyX3Block>(wg, A.st.x, A.st.y, c0);
        orun.place<kPolicyX3Block>(wg, A.st.x, A.st.y, c0, len, list,
                                   reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(smem) + wo));
        ord = list;
        nxt = load_env(tile < my_tiles ? tile : 0);
    }
    X3STAMP_ANY(10);
    const LdsWorld w = world_view(A.dims, A.world);  // port_at / stocks read in place (L2)
    const uint8_t* qb = reinterpret_cast<const uint8_t*>(smem);
    const float* W1 = reinterpret_cast<const float*>(qb + D.w1());
    const bf16x8* W2 = reinterpret_cast<const bf16x8*>(qb + D.w2());
    const bf16x8* W3 = reinterpret_cast<const bf16x8*>((kW3Global ? reinterpret_cast<const uint8_t*>(A.qimg) : qb) + D.w3());
    [[maybe_unused]] const float* B1 = reinterpret_cast<const float*>(qb + D.b1());
    const float* B2 = reinterpret_cast<const float*>(qb + D.b2());
    const float* B3 = reinterpret_cast<const float*>(qb + D.b3());
    const uint64_t* SAME = reinterpret_cast<const uint64_t*>(qb + D.same());
    const uint32_t* REGM = reinterpret_cast<const uint32_t*>(qb + D.regm());

    const int P = q.P;
    // the env state of the wave's next tile is loaded while this one computes (no HBM round
    // trip at the top of a tile), and its validity (the port on the ship's cell and that
    // port's stocks, two dependent L2 reads of the world image) resolved during fc3
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) >= 4) __builtin_amdgcn_s_setprio(1);
    EnvValid vnxt = env_valid(w, q, SAME, (int)nxt.x8(), (int)nxt.y8(), nxt.o8() == SE_NONE ? -1 : (int)nxt.o8());
    [[maybe_unused]] int tile_iter = 0;  // SHIPENV_X3_TRACE: the wave's 4th tile is stamped
    while (tile < my_tiles) {
        X3STAMP(0);
        const EnvIn in = nxt;
        const EnvValid v = vnxt;
        const int64_t tnext = tile + stride;
        const bool more = tnext < my_tiles;
        if (more) nxt = load_env(tnext);
        const int64_t e = in.e;
        const bool live = e < A.n;
        const double fuel = in.fuel;
        const uint32_t x8 = in.x8(), y8 = in.y8(), o8 = in.o8(), d8 = in.d8();
        const int origin = o8 == SE_NONE ? -1 : (int)o8, dest = d8 == SE_NONE ? -1 : (int)d8;
        const float ff = (float)fuel;  // the preprocess_state row as torch's FloatTensor holds it
        bf16x8 X1[4][2][3], X2[4][2][3];
        float best = -INFINITY;
        int bidx = 0x7fffffff;
        // The same arithmetic, hand-interleaved: the MFMAs go in groups of three (half a
        // k-step), and beside each group, fenced by sched_barrier so the compiler cannot
        // cluster them again, about five VALU of work that does not feed those MFMAs (a
        // chunk of a split of the layer's other tiles, or of the previous fc3 tile's
        // argmax). A wave's VALU then issues while its own MFMAs occupy the matrix pipe
        // (32 cycles each) instead of between MFMA phases. fc2 runs k-tile by k-tile over
        // its four row tiles (four accumulators), so k-tile kt + 1 is split during k-tile kt;
        // its last k-tile runs row tile by row tile, so the finished row tiles split beside
        // the rest; fc3's first tile splits fc2's last one. Fragments are read one k-step
        // ahead. Bit-identical to the plain order (the same operations on the same values).
        f32x16 c1[4], acc[4];
        bf16x8 xin[2];  // fc1's B operands: slot 16 step + 8h + j of x3_fc1_slot
        {
            __bf16 f0, f1, f2;
            split3(ff, f0, f1, f2);
            const __bf16 fp[3] = {f0, f1, f2};
            const __bf16 ex[6] = {(__bf16)(float)x8, (__bf16)(float)y8, f0, f0, (__bf16)(float)origin,
                                  (__bf16)(float)dest};  // exact inputs by column (2, 3 unused)
#pragma unroll
            for (int st = 0; st < 2; ++st)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const Fc1Slot a = x3_fc1_slot(16 * st + j), b = x3_fc1_slot(16 * st + 8 + j);
                    const __bf16 va = a.col == -2 ? (__bf16)1.0f : a.col < 0 ? (__bf16)0.0f : (a.xp < 0 ? ex[a.col] : fp[a.xp]);
                    const __bf16 vb = b.col == -2 ? (__bf16)1.0f : b.col < 0 ? (__bf16)0.0f : (b.xp < 0 ? ex[b.col] : fp[b.xp]);
                    xin[st][j] = h ? vb : va;
                }
        }
        const bf16x8* W1b = reinterpret_cast<const bf16x8*>(W1);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {  // fc1 (x, y | fuel, fuel | origin, dest)
            c1[mt] = bias_frag(B1 + mt * 32 + 4 * h);
            c1[mt] = mfma_bf16(W1b[(mt * 2 + 0) * 64 + lane], xin[0], c1[mt]);
            c1[mt] = mfma_bf16(W1b[(mt * 2 + 1) * 64 + lane], xin[1], c1[mt]);
            if (mt == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = bias_frag(B2 + i * 32 + 4 * h);
            } else {  // X1[0]'s 8 pairs beside fc1's other row tiles: 3, 3, 2
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if ((mt - 1) * 3 + j < 8) split_pair(c1[0], X1[0], (mt - 1) * 3 + j);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        X3STAMP(1);
        // fragments read kLa k-steps ahead over the flat k-step sequence: fc2's 32 (k-tile
        // kt, row tile mt, step s2), then fc3 tile 0's 8
        constexpr int kLa = 2;  // 1 / 3: 0.2582 / 0.2569 vs 0.2549 ms (profiles/r05/ab_policy_f32_la.jsonl)
        bf16x8 wf[kLa + 1][3];
        auto frag_of = [&](int j, bf16x8 (&dst)[3]) {
            if (j < 32) x3_frags(W2, (((j >> 1) & 3) * 4 + (j >> 3)) * 2 + (j & 1), lane, dst);
            else x3_frags(W3, j - 32, lane, dst);
        };
#pragma unroll
        for (int j = 0; j < kLa; ++j) frag_of(j, wf[j]);
        // the next tile's two dependent world reads (its cell code, then that port's stocks)
        // go out during fc2, so their round trips overlap the MFMAs
        int ncode = 0;
        int2 nstock = make_int2(0, 0);
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int kt = i >> 3, mt = (i >> 1) & 3, s2 = i & 1;
            if (i == 8) ncode = w.code((int)nxt.x8(), (int)nxt.y8());
            // unconditional (past the last tile nxt is tile 0's state, a valid address) and
            // opaque until their uses: under `if (more)` the compiler merged the arithmetic on
            // each into its load's block and waited out the round trip right there
            if (i == 24) {
                asm volatile("" : "+v"(ncode));
                nstock = w.stock[max(w.port_of_code(ncode), 0)];
            }
            if (i == 8) X3STAMP(2);
            if (i == 16) X3STAMP(3);
            if (i == 24) X3STAMP(4);
            frag_of(i + kLa, wf[(i + kLa) % (kLa + 1)]);
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                acc[mt] = khalf_x3(wf[i % (kLa + 1)], X1[kt][s2], acc[mt], half);
                const int g = 2 * (i & 7) + half;  // group within the k-tile, 0..15
                if (kt < 3) {
                    if (half == 0) split_pair(c1[kt + 1], X1[kt + 1], g >> 1);  // 8 pairs over 16 groups
                } else if (mt > 0) {  // the previous row tile's 8 pairs over this row tile's 4 groups
                    split_pair(acc[mt - 1], X2[mt - 1], 2 * (g - 4 * mt));
                    split_pair(acc[mt - 1], X2[mt - 1], 2 * (g - 4 * mt) + 1);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // fc3 tile 0 (the moves: every env can choose from it), fc2's last row tile split
        // beside its first 8 groups (done before k-step 6 reads it). Without q_out, a row
        // no action of this env can take starts at -inf (masked_bias), so the argmax needs
        // no validity test and never picks it.
        X3STAMP(5);
        auto mask_of = [&](int mt) { return tile_mask(v, mt, P); };
        // a tile of ships at sea only (uniform; ~3 in 4 under the visiting order) needs rows 0-3
        // (the moves) of fc3 tile 0: its six part products go as three chains, one per
        // activation part x_j, each over the weight parts w_p with p + j <= 2 stacked in the
        // MFMA's rows (x0: w0, w1, w2 in rows 0-3, 4-7, 8-11; x1: w0, w1; x2: w0; the other
        // rows read a zero row of the image), 24 MFMAs where the tile takes 48. Q(row r) = rows
        // r + (4 + r) + (8 + r): the same six products per k-step, summed by chain (an fp32
        // rounding per MFMA as before, in another order: not the same bits as the full tile).
        // 0.2409 -> 0.2275 ms per call at 2^20 (profiles/r06/order/ab_x3_stack.jsonl); the LDS
        // image only (the global-image variant would spill).
        const bool stack = !kW3Global && !kQout && D.zrow >= 0 && !__any(v.cur >= 0);
        f32x16 c;
        if (stack) {
            c = f32x16{};
            if (h == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) c[i] = B3[i];
            }
            const int r = lane & 31;
            // bf16x8 index of k-step 0's operand for chain j (k-step k adds 192)
            const int zero = D.zrow + 32 * h;
            const int src = (r >> 2) * 64 + (r & 3) + 32 * h;
            const int o0 = r < 12 ? src : zero, o1 = r < 8 ? src : zero, o2 = r < 4 ? src : zero;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const bf16x8 a2 = W3[k * 192 + o2], a1 = W3[k * 192 + o1], a0 = W3[k * 192 + o0];
                c = mfma_bf16(a2, X2[k >> 1][k & 1][2], c);
                c = mfma_bf16(a1, X2[k >> 1][k & 1][1], c);
                c = mfma_bf16(a0, X2[k >> 1][k & 1][0], c);
                if (k < 4) {  // X2[3] complete before k-step 6 reads it
                    split_pair(acc[3], X2[3], 2 * k);
                    split_pair(acc[3], X2[3], 2 * k + 1);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            c = kQout ? bias_frag(B3 + 4 * h) : masked_bias(B3 + 4 * h, mask_of(0) >> (4 * h));
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (32 + k + kLa < 40) frag_of(32 + k + kLa, wf[(32 + k + kLa) % (kLa + 1)]);
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    c = khalf_x3(wf[(32 + k) % (kLa + 1)], X2[k >> 1][k & 1], c, half);
                    const int g = 2 * k + half;
                    if (g < 8) split_pair(acc[3], X2[3], g);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        X3STAMP(6);
        // the next tile's validity from the world reads issued during fc2 (ncode, nstock)
        // waited for here on every path: a wait only inside env_valid_from's port branch left
        // the load outstanding into the next tile, whose first write of its registers then
        // waited out the new env loads as well
        asm volatile("" ::"v"(nstock.x), "v"(nstock.y));
        vnxt = env_valid_from(w, q, SAME, ncode, nstock, nxt.o8() == SE_NONE ? -1 : (int)nxt.o8());
        // fc3 tiles 1..: the previous tile's argmax beside each chain, 4 registers a group
        int pbase = 0;
        [[maybe_unused]] float best0 = best;
        [[maybe_unused]] int bt = 0;
        uint32_t pm = kQout ? tile_mask(v, 0, P) : 0u, prm = __builtin_amdgcn_readfirstlane(REGM[0]);
        if (kQout && live) tile_q_out(A.q_out, A.ldq, q.rows, c, e, 0, h, ff);
#pragma nounroll
        for (int mt = 1; mt < q.mt3; ++mt) {
            const int base = mt * 32;
            const uint32_t m3 = kQout ? 0u : mask_of(mt);
            if (!kQout && !__any(tile_maybe(v, mt, P))) continue;
            const bf16x8* W3t = W3 + mt * 8 * 192;
            f32x16 c3 = kQout ? bias_frag(B3 + mt * 32 + 4 * h) : masked_bias(B3 + mt * 32 + 4 * h, m3 >> (4 * h));
#pragma unroll
            for (int j = 0; j < kLa; ++j) x3_frags(W3t, j, lane, wf[j]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k + kLa < 8) x3_frags(W3t, k + kLa, lane, wf[(k + kLa) % (kLa + 1)]);
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    c3 = khalf_x3(wf[k % (kLa + 1)], X2[k >> 1][k & 1], c3, half);
                    const int g = 2 * k + half;
                    if (g < 4) {
                        if (kQout) {
                            tile_argmax_part(c, pm, prm, pbase, h, best, bidx, g);
                        } else {
                            if (g == 0) best0 = best;
                            argmax_local_part(c, best, bt, g);
                            if (g == 3) bidx = best != best0 ? pbase + bt : bidx;
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            c = c3;
            pbase = base;
            if (kQout) pm = tile_mask(v, mt, P);
            prm = __builtin_amdgcn_readfirstlane(REGM[mt]);
            if (kQout && live) tile_q_out(A.q_out, A.ldq, q.rows, c, e, base, h, ff);
        }
        X3STAMP(7);
        if (kQout) {
            tile_argmax(c, pm, prm, pbase, h, best, bidx);
        } else if (stack) {  // rows 0-3 from the three chains' partial rows
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float qi = (c[i] + __shfl_xor(c[i], 32)) + c[4 + i];
                const bool better = qi > best;  // ascending rows: the first maximum
                best = better ? qi : best;
                bidx = better ? i : bidx;
            }
            best = h ? -INFINITY : best;  // lane half 1 holds no row of its own
            bidx = h ? 0x7fffffff : bidx;
        } else {
            best0 = best;
#pragma unroll
            for (int g = 0; g < 4; ++g) argmax_local_part(c, best, bt, g);
            bidx = best != best0 ? pbase + bt : bidx;
            bidx += bidx == 0x7fffffff ? 0 : 4 * h;  // the lane half's rows (argmax_local_part omits 4h)
        }
        FINISH_ENV(v, e, live, h, best, bidx, x8, y8, o8, d8, ff);
        X3STAMP(8);
        tile = more ? tnext : my_tiles;
        ++tile_iter;
    }
    X3STAMP_ANY(11);
}
