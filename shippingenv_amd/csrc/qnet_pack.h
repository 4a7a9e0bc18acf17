#pragma once
// qnet_pack.h — the packers of the network images: qnet_pack_kernel (the bf16 image, both fc3
// layouts in one launch) and pack_x3_items (the split-bf16 image; qnet_pack_x3_kernel runs it
// over global memory, policy_x3_kernel over its own LDS), with the fc1 bias fold x3_fold_b1.
//
// A fragment of shipenv.hip's translation unit, included inside qpolicy.h's anonymous
// namespace after qnet_parts.h: not a stand-alone header. Uses qnet_image.h (the layouts, fc1_col,
// acc_row, x3_fc1_slot), qnet_parts.h (the vector types, split3) and world.h (WorldDims, LdsWorld,
// world_view).

// ------------------------------------------------------------------ packing
// One thread per 16-byte fragment slot / bias entry. Fragment (tile, step) lane
// (r = lane & 31, h = lane >> 5) element j holds W[tile*32 + r][k] with
//   fc1: k = column map of j (h = 0 only; the obs fragment below uses the same map)
//   fc2, fc3: k = kt*32 + 16s + 8(j >> 2) + 4h + (j & 3), the row of the previous
//   layer's accumulator that register 8s + j of lane half h holds.
struct PackArgs {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    const uint32_t* world;
    WorldDims dims;
    QnetDims q[2];  // blockIdx.y: the full layout, the compact one
    uint8_t* img[2];
    int32_t* bump;  // se_qnet_repack: a device counter advanced once, or null
};

__global__ __launch_bounds__(256) void qnet_pack_kernel(PackArgs A) {
    const QnetDims q = A.q[blockIdx.y];
    uint8_t* const img = A.img[blockIdx.y];
    if (A.bump && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *A.bump += 1;
    const int in1 = q.in1();
    const int n_w1 = 4 * 64, n_w2 = 32 * 64, n_w3 = q.mt3 * 8 * 64;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x;
         t < n_w1 + n_w2 + n_w3 + 2 * kQHidden + q.mt3 * 32 + q.P + q.mt3; t += gridDim.x * blockDim.x) {
        if (t < n_w1 + n_w2 + n_w3) {
            int f = t >> 6;
            const int lane = t & 63, r = lane & 31, h = lane >> 5;
            bf16x8 v;
            uint8_t* dst;
            if (t < n_w1) {  // fc1 tile f
                const int row = f * 32 + r;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = h == 0 ? (__bf16)A.w1[row * in1 + fc1_col(j)] : (__bf16)0.0f;
                dst = img + q.w1() + f * 1024 + lane * 16;
            } else {
                const bool second = t < n_w1 + n_w2;
                f -= second ? 4 : 4 + 32;  // fragment index ((mt*4 + kt)*2 + s)
                const int s = f & 1, kt = (f >> 1) & 3, mt = f >> 3;
                const int row = mt * 32 + r;
                const float* W = second ? A.w2 : A.w3;
                const bool in = second || row < q.rows;
                const int wrow = second ? row : q.action_of_row(row);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    v[j] = in ? (__bf16)W[wrow * kQHidden + kt * 32 + acc_row(s, j, h)] : (__bf16)0.0f;
                dst = img + (second ? q.w2() : q.w3()) + f * 1024 + lane * 16;
            }
            *reinterpret_cast<bf16x8*>(dst) = v;
            continue;
        }
        // (this tail stands in pack_x3_items too: as one function it changed both pack kernels' code)
        int u = t - (n_w1 + n_w2 + n_w3);
        const LdsWorld wv = world_view(A.dims, A.world);  // the device image, read in place
        const uint32_t* pos = wv.pos;
        const int P = q.P;
        if (u < kQHidden) {  // b1 + fc1 over the constant port block (x, y, fuel, cargo per port)
            double acc = (double)A.b1[u];
            for (int p = 0; p < P; ++p) {
                const float* w = A.w1 + u * in1 + 6 + 4 * p;
                acc += (double)w[0] * (double)wv.px(p) + (double)w[1] * (double)wv.py(p) +
                       (double)w[2] * (double)wv.pfuel(p) + (double)w[3] * (double)wv.pcargo(p);
            }
            reinterpret_cast<float*>(img + q.b1())[u] = (float)acc;
        } else if ((u -= kQHidden) < kQHidden) {
            reinterpret_cast<float*>(img + q.b2())[u] = A.b2[u];
        } else if ((u -= kQHidden) < q.mt3 * 32) {
            reinterpret_cast<float*>(img + q.b3())[u] = u < q.rows ? A.b3[q.action_of_row(u)] : 0.0f;
        } else if ((u -= q.mt3 * 32) < P) {  // bit p: port p stands on port u's cell (u included)
            uint64_t same = 0;
            for (int p = 0; p < P; ++p)
                if (pos[p] == pos[u]) same |= 1ull << p;
            reinterpret_cast<uint64_t*>(img + q.same())[u] = same;
        } else {
            // fc3 tile mt = u - P: bit reg set when accumulator register reg (rows
            // base + (reg & 3) + 8 (reg >> 2) + 4h, h = 0, 1) can hold a valid action of
            // ANY env: a move or SELECT (row < 4 + P), or an amount within the largest
            // stock (is_valid_action, dqn.py:125-175). The epilogue skips the others.
            const int mt = u - P, base = mt * 32;
            int cmax = 0, fmax = 0;
            for (int p = 0; p < P; ++p) {
                cmax = max(cmax, min(wv.pcargo(p), 49));
                fmax = max(fmax, min(wv.pfuel(p), 199));
            }
            const int c_lo = 5 + P, c_hi = 4 + P + cmax, f_lo = 55 + P, f_hi = 54 + P + fmax;
            uint32_t rm = 0;
            for (int reg = 0; reg < 16; ++reg)
                for (int h = 0; h < 2; ++h) {
                    const int row = base + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                    const int a = q.action_of_row(row);
                    const bool ok = row < q.rows && (a < 4 + P || (a >= c_lo && a <= c_hi) ||
                                                     (a >= f_lo && a <= f_hi));
                    rm |= (uint32_t)ok << reg;
                }
            reinterpret_cast<uint32_t*>(img + q.regm())[mt] = rm;
        }
    }
}

constexpr int kX3PtabBytes = 3 * 64 * 4 + 16;  // the staged port table, past the image

struct PackX3Args {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    const uint32_t* world;
    WorldDims dims;
    QnetX3Dims d;
    uint8_t* img;
    // policy_x3_kernel's own pack: the port table (P positions, then P
    // stock pairs) staged in LDS, so the b1 folds and the same-cell / register masks read it
    // there instead of looping over L2 loads; null: the world image in place
    const uint32_t* ptab = nullptr;
};

// the world view the pack reads the ports through
__device__ __forceinline__ LdsWorld pack_world(const PackX3Args& A) {
    LdsWorld wv = world_view(A.dims, A.world);
    if (A.ptab) {
        wv.pos = A.ptab;
        wv.stock = reinterpret_cast<const int2*>(A.ptab + 64);
    }
    return wv;
}

// One thread per (fragment, lane) of fc2 / fc3 (its 8 elements' three parts), per fc1 float,
// bias entry, same-cell mask and epilogue register mask (the latter as qnet_pack_kernel).
// items [first, total) step `stride` of the split image into img (global memory for
// qnet_pack_x3_kernel, the workgroup's LDS for policy_x3_kernel's own prologue)
// b1[f] + W1[f, 6:] . the port block, in f64 then f32 (qnet_pack_kernel's fold)
__device__ __forceinline__ float x3_fold_b1(const PackX3Args& A, int f) {
    const LdsWorld wv = pack_world(A);
    const int in1 = A.d.q.in1();
    double acc = (double)A.b1[f];
    // unrolled so that several ports' weight loads go out before the adds wait on them (the
    // adds stay in port order; unroll 8 measured even, profiles/r05/ab_policy_f32_fold_unroll.jsonl;
    // all 8 ports' loads issued before the adds measured even too, profiles/r06/order/ab_x3_fold.jsonl)
#pragma unroll 1
    for (int p = 0; p < A.d.q.P; ++p) {
        const float* w = A.w1 + f * in1 + 6 + 4 * p;
        acc += (double)w[0] * (double)wv.px(p) + (double)w[1] * (double)wv.py(p) + (double)w[2] * (double)wv.pfuel(p) +
               (double)w[3] * (double)wv.pcargo(p);
    }
    return (float)acc;
}

__device__ __forceinline__ void pack_x3_items(const PackX3Args& A, uint8_t* img, int first, int stride) {
    const QnetX3Dims d = A.d;
    const QnetDims q = d.q;
    const int in1 = q.in1();
    const int n_w1 = 4 * 2 * 64, n_w2 = 32 * 64, n_w3 = q.mt3 * 8 * 64;
    const int total = n_w1 + n_w2 + n_w3 + 2 * kQHidden + q.mt3 * 32 + q.P + q.mt3;
    // fc2 / fc3 fragments first, in a loop of their own: an item's 8 weights are two float4
    // loads (elements 0-3 and 4-7 are consecutive columns), split as pairs, and 6 items' loads
    // go out together (0.2646 -> 0.2613 ms per call against 2,
    // profiles/r05/ab_policy_f32_pack_unroll.jsonl). Same bits as the
    // per-element split3 below. Taken when both weight matrices are 16-byte aligned (torch's
    // allocations are); otherwise the element-wise loop below packs them.
    const bool vec = ((reinterpret_cast<uintptr_t>(A.w2) | reinterpret_cast<uintptr_t>(A.w3)) & 15) == 0;
#pragma unroll 6
    for (int u0 = vec ? first : n_w2 + n_w3; u0 < n_w2 + n_w3; u0 += stride) {
        const bool second = u0 < n_w2;
        const int u = second ? u0 : u0 - n_w2;
        const int f = u >> 6, lane = u & 63, r = lane & 31, h = lane >> 5;
        const int s = f & 1, kt = (f >> 1) & 3, mt = f >> 3;
        const int row = mt * 32 + r;
        const bool in = second || row < q.rows;
        const float* W = second ? A.w2 : A.w3;
        const int wrow = second ? row : (in ? q.action_of_row(row) : 0);
        const float4* src = reinterpret_cast<const float4*>(W + wrow * kQHidden + kt * 32 + acc_row(s, 0, h));
        float4 a = src[0], b = src[2];  // columns acc_row(s, 0..3, h) and acc_row(s, 4..7, h) = +8
        if (!in) a = b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        u32x4 w[3];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const f32x2 x{v[2 * k], v[2 * k + 1]};  // (the pack, not beside MFMAs: packed subtractions)
            const bf16x2 p0 = __builtin_convertvector(x, bf16x2);
            const f32x2 r1 = x - __builtin_convertvector(p0, f32x2);
            const bf16x2 p1 = __builtin_convertvector(r1, bf16x2);
            const bf16x2 p2 = __builtin_convertvector(r1 - __builtin_convertvector(p1, f32x2), bf16x2);
            w[0][k] = __builtin_bit_cast(uint32_t, p0);
            w[1][k] = __builtin_bit_cast(uint32_t, p1);
            w[2][k] = __builtin_bit_cast(uint32_t, p2);
        }
        uint8_t* dst = img + (second ? d.w2() : d.w3()) + f * 3 * 1024 + lane * 16;
#pragma unroll
        for (int k = 0; k < 3; ++k) *reinterpret_cast<u32x4*>(dst + k * 1024) = w[k];
    }
    for (int t = first; t < total; t += stride) {
        if (vec && t >= n_w1 && t < n_w1 + n_w2 + n_w3) continue;  // packed above
        if (t < n_w1) {
            const int lane = t & 63;
            // fc1 fragment (mt, step, lane): element j = slot 16 step + 8h + j
            const int st = (t >> 6) & 1, mt = t >> 7, row = mt * 32 + (lane & 31);
            bf16x8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const Fc1Slot sl = x3_fc1_slot(16 * st + 8 * (lane >> 5) + j);
                __bf16 p0 = (__bf16)0.0f, p1 = p0, p2 = p0;
                if (sl.col >= 0) split3(A.w1[row * in1 + sl.col], p0, p1, p2);
                v[j] = sl.wp == 0 ? p0 : (sl.wp == 1 ? p1 : p2);
            }
            reinterpret_cast<bf16x8*>(img + d.w1())[t] = v;
            continue;
        }
        if (t < n_w1 + n_w2 + n_w3) {  // fragment f = (mt*4 + kt)*2 + s, lane: W[row][kt*32 + acc_row(s, j, h)]
            const bool second = t < n_w1 + n_w2;
            const int u = t - (second ? n_w1 : n_w1 + n_w2);
            const int f = u >> 6, lane = u & 63, r = lane & 31, h = lane >> 5;
            const int s = f & 1, kt = (f >> 1) & 3, mt = f >> 3;
            const int row = mt * 32 + r;
            const bool in = second || row < q.rows;
            const float* W = second ? A.w2 : A.w3;
            const int wrow = second ? row : q.action_of_row(row);
            bf16x8 p[3];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = in ? W[wrow * kQHidden + kt * 32 + acc_row(s, j, h)] : 0.0f;
                __bf16 a, b, c;
                split3(v, a, b, c);
                p[0][j] = a;
                p[1][j] = b;
                p[2][j] = c;
            }
            uint8_t* dst = img + (second ? d.w2() : d.w3()) + f * 3 * 1024 + lane * 16;
#pragma unroll
            for (int k = 0; k < 3; ++k) *reinterpret_cast<bf16x8*>(dst + k * 1024) = p[k];
            continue;
        }
        int u = t - (n_w1 + n_w2 + n_w3);
        const LdsWorld wv = pack_world(A);
        const int P = q.P;
        if (u < kQHidden) {  // b1 + fc1 over the constant port block, in f64 then f32
            reinterpret_cast<float*>(img + d.b1())[u] = x3_fold_b1(A, u);
        } else if ((u -= kQHidden) < kQHidden) {
            reinterpret_cast<float*>(img + d.b2())[u] = A.b2[u];
        } else if ((u -= kQHidden) < q.mt3 * 32) {
            reinterpret_cast<float*>(img + d.b3())[u] = u < q.rows ? A.b3[q.action_of_row(u)] : 0.0f;
        } else if ((u -= q.mt3 * 32) < P) {
            uint64_t same = 0;
            for (int p = 0; p < P; ++p)
                if (wv.pos[p] == wv.pos[u]) same |= 1ull << p;
            reinterpret_cast<uint64_t*>(img + d.same())[u] = same;
        } else {
            const int mt = u - P, base = mt * 32;
            int cmax = 0, fmax = 0;
            for (int p = 0; p < P; ++p) {
                cmax = max(cmax, min(wv.pcargo(p), 49));
                fmax = max(fmax, min(wv.pfuel(p), 199));
            }
            const int c_lo = 5 + P, c_hi = 4 + P + cmax, f_lo = 55 + P, f_hi = 54 + P + fmax;
            uint32_t rm = 0;
            for (int reg = 0; reg < 16; ++reg)
                for (int h = 0; h < 2; ++h) {
                    const int row = base + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                    const int a = q.action_of_row(row);
                    const bool ok = row < q.rows && (a < 4 + P || (a >= c_lo && a <= c_hi) || (a >= f_lo && a <= f_hi));
                    rm |= (uint32_t)ok << reg;
                }
            reinterpret_cast<uint32_t*>(img + d.regm())[mt] = rm;
        }
    }
}

__global__ __launch_bounds__(256) void qnet_pack_x3_kernel(PackX3Args A) {
    pack_x3_items(A, A.img, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}
