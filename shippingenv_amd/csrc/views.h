#pragma once
// views.h — the kernels beside the step: the done list's contiguous copy
// (done_scan_kernel, done_copy_kernel), reset_kernel, the two observe kernels, the
// three valid-mask kernels with their row templates, and gen_actions_kernel.
//
// A fragment of shipenv.hip's translation unit, included inside its anonymous
// namespace where this text stood: not a stand-alone header.
// Uses world.h (LdsWorld, stage_world, world_view), env_core.h (Ship, env_key,
// reset_ship) and step_io.h (st_stream).

// Contiguous copy of the last step's done lists (se_done_compact), in two launches:
// done_scan_kernel (one workgroup) turns the per-segment counts into exclusive
// offsets, chunk by chunk in segment order; done_copy_kernel copies segment s to
// out[offsets[s]...], one wave per segment.
__global__ __launch_bounds__(1024) void done_scan_kernel(const int32_t* __restrict__ counts, int64_t nseg,
                                                         int32_t* __restrict__ offsets,
                                                         int32_t* __restrict__ out_count) {
    __shared__ int32_t part[1024];
    const int64_t chunk = (nseg + 1023) / 1024;
    const int64_t lo = (int64_t)threadIdx.x * chunk, hi = lo + chunk < nseg ? lo + chunk : nseg;
    int32_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += counts[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {  // inclusive Hillis-Steele scan of the chunk sums
        const int32_t v = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int32_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (int64_t i = lo; i < hi; ++i) {
        offsets[i] = run;
        run += counts[i];
    }
    if (threadIdx.x == 1023) *out_count = part[1023];
}

__global__ __launch_bounds__(kBlock) void done_copy_kernel(const se_done_rec* __restrict__ recs,
                                                           const int32_t* __restrict__ counts,
                                                           const int32_t* __restrict__ offsets, int64_t nseg,
                                                           int64_t seg, se_done_rec* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (s >= nseg) return;
    const int32_t cnt = counts[s], start = offsets[s];
    for (int i = threadIdx.x & 63; i < cnt; i += 64) out[start + i] = recs[s * seg + i];
}

// ------------------------------------------------------------------ reset kernel
struct ResetArgs {
    const uint32_t* world;
    WorldDims dims;
    int64_t n, env_base;
    uint64_t seed;
    uint32_t epoch;
    uint32_t t;  // the step counter: the first step of the new episodes
    se_state st;
    const uint8_t* mask;
    const int32_t* origin_in;  // explicit values (se_reset_to) or NULL
    const int32_t* dest_in;
};

// The world is read in place (only the port positions, for the envs being reset): staged
// per workgroup as the other kernels do, it cost 2048 x 10.8 KB of L2 reads per launch,
// the whole launch when a mask selects a few envs (the training loop's episode cuts).
__device__ __forceinline__ void reset_env(const ResetArgs& A, const LdsWorld& w, int64_t i) {
    {
        Ship s;
        if (A.origin_in) {
            s.origin = A.origin_in[i];
            s.dest = A.dest_in[i];
            s.cargo = 0;
            s.fuel = kFuelInit;
            s.x = w.px(s.origin);
            s.y = w.py(s.origin);
        } else {
            const U4 o = draw(env_key(A.seed, A.env_base + i), A.epoch, kSlotExplicitReset);
            reset_ship(w, s, o.v[0], o.v[1]);
        }
        store_ship(A.st, i, s);
        if (A.st.ep_return) A.st.ep_return[i] = 0.0f;
        if (A.st.ep_start) A.st.ep_start[i] = (int32_t)A.t;
        A.st.done[i] = 0;
        A.st.err[i] = 0;
        A.st.reward[i] = 0.0f;
    }
}

__global__ __launch_bounds__(kBlock) void reset_kernel(ResetArgs A) {
    const LdsWorld w = world_view(A.dims, A.world);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < A.n;
         i += (int64_t)gridDim.x * kBlock) {
        if (A.mask && !A.mask[i]) continue;
        reset_env(A, w, i);
    }
}

// ------------------------------------------------------------------ observation
// preprocess_state rows (utils/preprocessing.py:25-62): one thread per output
// element so the f32 row writes are coalesced; the port block comes from LDS.
struct ObsArgs {
    const uint32_t* world;
    WorldDims dims;
    int64_t n, ld;
    se_state st;
    float* obs;
};

__global__ __launch_bounds__(kBlock) void observe_kernel(ObsArgs A) {
    extern __shared__ uint32_t lds[];
    const LdsWorld w = stage_world(A.world, A.dims, lds);
    const int64_t width = 6 + 4 * (int64_t)w.P;
    const int64_t total = A.n * width;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < total;
         k += (int64_t)gridDim.x * kBlock) {
        const int64_t i = k / width;
        const int c = (int)(k - i * width);
        float v;
        if (c < 6) {
            switch (c) {
            case 0: v = (float)A.st.x[i]; break;
            case 1: v = (float)A.st.y[i]; break;
            case 2:
            case 3: v = (float)A.st.fuel[i]; break;  // "cargo" is self.fuel (environment.py:206)
            case 4: v = A.st.origin[i] == SE_NONE ? -1.0f : (float)A.st.origin[i]; break;
            default: v = A.st.dest[i] == SE_NONE ? -1.0f : (float)A.st.dest[i]; break;
            }
        } else {
            const int p = (c - 6) >> 2, f = (c - 6) & 3;
            v = f == 0 ? (float)w.px(p) : f == 1 ? (float)w.py(p) : f == 2 ? (float)w.pfuel(p) : (float)w.pcargo(p);
        }
        A.obs[i * A.ld + c] = v;
    }
}

// Rows of a 256-row tile are contiguous in a dense [n][W] output, so a workgroup
// builds its tile's values once and writes them with 16-byte stores in address order
// (every wave store a full 1 KB run). The generic kernels above / below (one thread per
// output element or byte) serve any other row stride; they measured 117 us (observe,
// P = 5) and 321 us (mask) at 2^20 envs against 22 us and 7 us of HBM writes.
constexpr int kTileRows = 256;  // = kBlock: one row per thread in the per-row phase

// x / W for x < kTileRows * W, W <= 1022, as one multiply-high (exact: checked for every
// such x and W)
__device__ __forceinline__ uint32_t div_tile(uint32_t x, uint32_t magic) { return __umulhi(x, magic); }

// preprocess_state rows, dense ld == W = 6 + 4P: the tile's ship columns (6 floats a row)
// and the constant port block (4P floats) in LDS, then float4 stores
__global__ __launch_bounds__(kBlock) void observe_tiled_kernel(ObsArgs A, uint32_t magic) {
    extern __shared__ float olds[];
    const LdsWorld w = world_view(A.dims, A.world);  // only the port table is read
    const int W = 6 + 4 * w.P;
    float* ship = olds;                  // [kTileRows][6]
    float* pblk = olds + kTileRows * 6;  // [4P]
    for (int c = threadIdx.x; c < 4 * w.P; c += kBlock) {
        const int p = c >> 2, f = c & 3;
        pblk[c] = f == 0 ? (float)w.px(p) : f == 1 ? (float)w.py(p) : f == 2 ? (float)w.pfuel(p) : (float)w.pcargo(p);
    }
    for (int64_t r0 = (int64_t)blockIdx.x * kTileRows; r0 < A.n; r0 += (int64_t)gridDim.x * kTileRows) {
        const int rows = (int)min((int64_t)kTileRows, A.n - r0);
        __syncthreads();  // the previous tile's reads of `ship` are done
        if ((int)threadIdx.x < rows) {
            const int64_t i = r0 + threadIdx.x;
            const float fuel = (float)A.st.fuel[i];  // "cargo" is self.fuel (environment.py:206)
            const uint8_t o = A.st.origin[i], d = A.st.dest[i];
            float* sr = ship + threadIdx.x * 6;
            sr[0] = (float)A.st.x[i];
            sr[1] = (float)A.st.y[i];
            sr[2] = fuel;
            sr[3] = fuel;
            sr[4] = o == SE_NONE ? -1.0f : (float)o;
            sr[5] = d == SE_NONE ? -1.0f : (float)d;
        }
        __syncthreads();
        const uint32_t nf = (uint32_t)(rows * W);  // W is even: whole float4 runs when rows is
        float4* out = reinterpret_cast<float4*>(A.obs + r0 * W);
        for (uint32_t q = threadIdx.x; 4 * q < nf; q += kBlock) {
            const uint32_t j = 4 * q;
            uint32_t r = div_tile(j, magic);
            int c = (int)(j - r * W);
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = c < 6 ? ship[r * 6 + c] : pblk[c - 6];
                if (++c == W) {
                    c = 0;
                    ++r;
                }
            }
            if (j + 4 <= nf) {
                out[q] = make_float4(v[0], v[1], v[2], v[3]);
            } else {  // the last run of a ragged tile: 2 floats (rows * W is even)
                A.obs[r0 * W + j] = v[0];
                A.obs[r0 * W + j + 1] = v[1];
            }
        }
    }
}

// ------------------------------------------------------------------ DQN validity mask
// agents/dqn.py:125-175, one thread per output byte (8 agent indices).
struct MaskArgs {
    const uint32_t* world;
    WorldDims dims;
    int64_t n;
    int32_t stride;
    se_state st;
    uint8_t* bits;
};

__global__ __launch_bounds__(kBlock) void valid_mask_kernel(MaskArgs A) {
    extern __shared__ uint32_t lds[];
    const LdsWorld w = stage_world(A.world, A.dims, lds);
    const int P = w.P, nact = 4 + P + 250;
    const int64_t total = A.n * A.stride;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < total;
         k += (int64_t)gridDim.x * kBlock) {
        const int64_t i = k / A.stride;
        const int byte = (int)(k - i * A.stride);
        const int x = A.st.x[i], y = A.st.y[i];
        const int origin = A.st.origin[i] == SE_NONE ? -1 : A.st.origin[i];
        const int cur = w.port_at(x, y);
        uint32_t out = 0;
        for (int bit = 0; bit < 8; ++bit) {
            const int a = byte * 8 + bit;
            bool v;
            if (a >= nact) v = false;
            else if (a < 4) v = true;
            else if (a < 4 + P) {
                const int p = a - 4;
                v = p != origin && w.px(p) == x && w.py(p) == y;
            } else if (a < 4 + P + 50) {
                const int amt = a - (4 + P);
                v = cur >= 0 && amt > 0 && amt <= w.pcargo(cur);
            } else {
                const int amt = a - (4 + P + 50);
                v = cur >= 0 && amt > 0 && amt <= w.pfuel(cur);
            }
            out |= (uint32_t)v << (7 - bit);
        }
        A.bits[k] = (uint8_t)out;
    }
}

// bits i of [0, 32) with lo <= i <= hi (lo, hi any ints)
__device__ __forceinline__ uint32_t bits_in(int lo, int hi) {
    lo = max(lo, 0);
    hi = min(hi, 31);
    if (lo > hi) return 0u;
    const uint32_t top = hi >= 31 ? 0xffffffffu : ((1u << (hi + 1)) - 1u);
    return top & ~((1u << lo) - 1u);
}

// is_valid_action bits, dense rows of S bytes: each thread builds its row 32 actions at a
// time (a word whose bit o is action 32k + o, then bit-reversed and byte-swapped into the
// MSB-first byte order of np.packbits), writes its S bytes into the LDS tile, then the
// workgroup stores the tile with 16-byte writes.
__global__ __launch_bounds__(kBlock) void valid_mask_tiled_kernel(MaskArgs A) {
    extern __shared__ uint8_t mlds[];  // [kTileRows][S] (+ pad to 16 bytes)
    __shared__ uint64_t same[64];  // P <= 64: bit q of same[p] = port q stands on port p's cell
    const LdsWorld w = world_view(A.dims, A.world);
    const int P = w.P, S = A.stride, nw = (S + 3) / 4;
    const int c_lo = 5 + P, f_lo = 55 + P;  // TAKE_CARGO / TAKE_FUEL amount 1
    const bool masks = P <= 64;  // the SELECT rows as one shifted mask per env (else a scan)
    if (masks && (int)threadIdx.x < P) {
        uint64_t m = 0;
        for (int q = 0; q < P; ++q) m |= (uint64_t)(w.pos[q] == w.pos[threadIdx.x]) << q;
        same[threadIdx.x] = m;
    }
    for (int64_t r0 = (int64_t)blockIdx.x * kTileRows; r0 < A.n; r0 += (int64_t)gridDim.x * kTileRows) {
        const int rows = (int)min((int64_t)kTileRows, A.n - r0);
        __syncthreads();  // the previous tile's stores have read the LDS tile
        if ((int)threadIdx.x < rows) {
            const int64_t i = r0 + threadIdx.x;
            const int x = A.st.x[i], y = A.st.y[i];
            const int origin = A.st.origin[i] == SE_NONE ? -1 : A.st.origin[i];
            const int cur = w.port_at(x, y);  // the first port on the ship's cell
            const int cst = cur >= 0 ? w.pcargo(cur) : 0, fst = cur >= 0 ? w.pfuel(cur) : 0;
            const uint32_t spos = (uint32_t)x | ((uint32_t)y << 16);
            // SELECT p: every port on the ship's cell but the origin (dqn.py:152-161)
            const uint64_t sel = masks && cur >= 0 ? same[cur] & ~(origin >= 0 ? 1ull << origin : 0ull) : 0ull;
            uint8_t* row = mlds + threadIdx.x * S;
            for (int k = 0; k < nw; ++k) {
                const int b = 32 * k;
                uint32_t m = bits_in(-b, 3 - b);  // moves: always
                if (cur >= 0) {
                    m |= bits_in(c_lo - b, c_lo + min(cst, 49) - 1 - b) | bits_in(f_lo - b, f_lo + min(fst, 199) - 1 - b);
                    if (masks) {  // rows 4 + p: sel shifted by 4 - b
                        const int sh = b - 4;
                        m |= (uint32_t)(sh < 0 ? sel << -sh : (sh < 64 ? sel >> sh : 0ull));
                    } else {
                        const int p0 = max(cur, b - 4), p1 = min(P, b + 28);
                        for (int p = p0; p < p1; ++p)
                            if (w.pos[p] == spos && p != origin) m |= 1u << (4 + p - b);
                    }
                }
                const uint32_t word = __builtin_amdgcn_perm(0u, __builtin_bitreverse32(m), 0x00010203u);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * k + j < S) row[4 * k + j] = (uint8_t)(word >> (8 * j));
            }
        }
        __syncthreads();
        const uint32_t nb = (uint32_t)(rows * S);
        uint8_t* out = A.bits + r0 * S;
        const uint4* src = reinterpret_cast<const uint4*>(mlds);
        for (uint32_t q = threadIdx.x; 16 * q < nb; q += kBlock) {
            if (16 * q + 16 <= nb) {
                reinterpret_cast<uint4*>(out)[q] = src[q];
            } else {
                for (uint32_t b = 16 * q; b < nb; ++b) out[b] = mlds[b];
            }
        }
    }
}

// Row templates (round 5). A row of is_valid_action bits depends on the ship's state only
// through (cur, origin): cur = the first port on the ship's cell (-1 at sea) fixes the
// TAKE_* amounts (its stocks) and the SELECT rows (every port on its cell), and the origin
// clears its own SELECT bit when it stands on that cell (dqn.py:152-161). So every row is
// one of 1 + P + sum_p |same[p]| templates: template 0 the moves alone, 1 + p port p's
// cell with no origin on it, and 1 + P + pbase[p] + rank(o) port p's cell with origin o
// cleared. mask_tmpl_kernel builds them once per world image into a device buffer:
//   [0, 512)    same[64]: bit q of same[p] = port q stands on port p's cell
//   [512, 772)  pbase[65]: prefix counts of |same[p]|
//   [1024, ...) ntmpl blocks of TB bytes: 16 zero bytes, the S row bytes in np.packbits
//               order, then zeros to the block's end (TB = round16(S + 35))
// so that a 16-byte window read at any byte offset of [0, 16 + S) of a block holds the
// row's bytes from that offset on, zeros before the row and after it.
constexpr int kMaskHdr = 1024;
__host__ __device__ constexpr int mask_tb(int S) { return (S + 35 + 15) & ~15; }
constexpr int kMaskTmplMax = 320;  // templates held in LDS (P = 64 on distinct cells: 129)

// the bits of actions [b, b + 32) of a row (bit o = action b + o), in packbits byte order
__device__ __forceinline__ uint32_t mask_word(int b, int cur, int cst, int fst, uint64_t sel, int P) {
    uint32_t m = bits_in(-b, 3 - b);  // moves: always
    if (cur >= 0) {
        const int c_lo = 5 + P, f_lo = 55 + P;  // TAKE_CARGO / TAKE_FUEL amount 1
        m |= bits_in(c_lo - b, c_lo + min(cst, 49) - 1 - b) | bits_in(f_lo - b, f_lo + min(fst, 199) - 1 - b);
        const int sh = b - 4;  // rows 4 + p: sel shifted by 4 - b
        m |= (uint32_t)(sh < 0 ? (-sh < 64 ? sel << -sh : 0ull) : (sh < 64 ? sel >> sh : 0ull));
    }
    return __builtin_amdgcn_perm(0u, __builtin_bitreverse32(m), 0x00010203u);
}

__global__ __launch_bounds__(kBlock) void mask_tmpl_kernel(const uint32_t* world, WorldDims d, int S,
                                                           uint8_t* buf) {
    const LdsWorld w = world_view(d, world);
    const int P = w.P, TB = mask_tb(S);
    __shared__ uint64_t same[64];
    __shared__ uint32_t pbase[65];
    if ((int)threadIdx.x < P) {
        uint64_t m = 0;
        for (int q = 0; q < P; ++q) m |= (uint64_t)(w.pos[q] == w.pos[threadIdx.x]) << q;
        same[threadIdx.x] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        pbase[0] = 0;
        for (int p = 0; p < P; ++p) pbase[p + 1] = pbase[p] + (uint32_t)__popcll(same[p]);
    }
    __syncthreads();
    if ((int)threadIdx.x < 64) reinterpret_cast<uint64_t*>(buf)[threadIdx.x] = (int)threadIdx.x < P ? same[threadIdx.x] : 0ull;
    if ((int)threadIdx.x <= 64) reinterpret_cast<uint32_t*>(buf + 512)[threadIdx.x] = (int)threadIdx.x <= P ? pbase[threadIdx.x] : 0u;
    const int ntmpl = 1 + P + (int)pbase[P], wpt = TB / 4;
    uint32_t* out = reinterpret_cast<uint32_t*>(buf + kMaskHdr);
    for (int k = threadIdx.x; k < ntmpl * wpt; k += kBlock) {
        const int t = k / wpt, c = 4 * (k - t * wpt) - 16;  // the word's first row byte
        int cur = -1;
        uint64_t sel = 0;
        if (t >= 1 && t <= P) {
            cur = t - 1;
            sel = same[cur];
        } else if (t > P) {
            const uint32_t j = (uint32_t)(t - 1 - P);
            int p = 0;
            while (pbase[p + 1] <= j) ++p;
            uint64_t m = same[p];
            for (uint32_t r = j - pbase[p]; r > 0; --r) m &= m - 1;  // the rank-th port of the cell
            cur = p;
            sel = same[p] & ~(m & (~m + 1));
        }
        uint32_t word = 0;
        if (c >= 0 && c < S) {
            word = mask_word(8 * c, cur, cur >= 0 ? w.pcargo(cur) : 0, cur >= 0 ? w.pfuel(cur) : 0, sel, P);
            const int keep = S - c;  // bytes of the word inside the row
            if (keep < 4) word &= (1u << (8 * keep)) - 1u;
        }
        out[k] = word;
    }
}

// 16 bytes of LDS from any byte offset (the blocks leave 4 spare bytes past every window)
__device__ __forceinline__ uint4 lds_window(const uint32_t* l, uint32_t off) {
    const uint32_t a = off >> 2, sh = off & 3u;
    const uint32_t w0 = l[a], w1 = l[a + 1], w2 = l[a + 2], w3 = l[a + 3], w4 = l[a + 4];
    return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                      __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh));
}

// is_valid_action bits from the row templates: per 256-row tile, one thread per row looks up
// its template (desc: the block's byte offset in LDS), then one thread per 16-byte chunk of
// the tile's dense output ORs the windows of the (at most two) rows the chunk covers and
// stores it: S and 256 * S are such that a chunk never spans three rows or two tiles.
__global__ __launch_bounds__(kBlock) void valid_mask_tmpl_kernel(MaskArgs A, const uint8_t* __restrict__ buf,
                                                                 int ntmpl, uint32_t magic) {
    extern __shared__ uint32_t tl[];  // [ntmpl * TB / 4] templates
    __shared__ uint64_t same[64];
    __shared__ uint32_t pbase[64];
    __shared__ uint32_t desc[kTileRows + 1];
    const LdsWorld w = world_view(A.dims, A.world);
    const int P = w.P, S = A.stride, TB = mask_tb(S);
    {
        const uint4* src = reinterpret_cast<const uint4*>(buf + kMaskHdr);
        uint4* dst = reinterpret_cast<uint4*>(tl);
        for (int k = threadIdx.x; k < ntmpl * TB / 16; k += kBlock) dst[k] = src[k];
        if (threadIdx.x < 64) {
            same[threadIdx.x] = reinterpret_cast<const uint64_t*>(buf)[threadIdx.x];
            pbase[threadIdx.x] = reinterpret_cast<const uint32_t*>(buf + 512)[threadIdx.x];
        }
    }
    for (int64_t r0 = (int64_t)blockIdx.x * kTileRows; r0 < A.n; r0 += (int64_t)gridDim.x * kTileRows) {
        const int rows = (int)min((int64_t)kTileRows, A.n - r0);
        __syncthreads();  // the templates are in; the previous tile's chunks have read desc
        {
            uint32_t id = 0;
            if ((int)threadIdx.x < rows) {
                const int64_t i = r0 + threadIdx.x;
                const int cur = w.port_at(A.st.x[i], A.st.y[i]);
                const int o = A.st.origin[i];  // SE_NONE (255) is never on a cell
                if (cur >= 0) {
                    const uint64_t sm = same[cur];
                    const bool on = o < 64 && ((sm >> o) & 1ull);
                    id = on ? 1u + (uint32_t)P + pbase[cur] + (uint32_t)__popcll(sm & ((1ull << o) - 1ull))
                            : 1u + (uint32_t)cur;
                }
            }
            desc[threadIdx.x] = id * (uint32_t)TB;
            // read only for row 255 of a full tile, whose last chunk ends on the tile's end (256 * S is a
            // multiple of 16), so nx is -16 and the window is a block's zero prefix: any block start serves
            if (threadIdx.x == 0) desc[kTileRows] = 0;
        }
        __syncthreads();
        const uint32_t nb = (uint32_t)(rows * S);
        uint8_t* out = A.bits + r0 * S;
        for (uint32_t q = threadIdx.x; 16 * q < nb; q += kBlock) {
            const uint32_t c = 16 * q, r = div_tile(c, magic), c0 = c - r * (uint32_t)S;
            const uint4 a = lds_window(tl, desc[r] + 16u + c0);
            // the next row's bytes land at chunk offset S - c0; a window from before that
            // row's start reads its zero prefix (-16 at most: otherwise the chunk ends first)
            const int nx = max((int)c0 - S, -16);
            const uint4 b = lds_window(tl, desc[r + 1] + (uint32_t)(16 + nx));
            const uint4 v = make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w);
            if (c + 16 <= nb) {
                st_stream(reinterpret_cast<uint4*>(out + c), v);
            } else {  // the ragged tail of the last tile
                const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
                for (uint32_t k = 0; c + k < nb; ++k) out[c + k] = (uint8_t)(vv[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

// ------------------------------------------------------------------ synthetic agent
__global__ __launch_bounds__(kBlock) void gen_actions_kernel(int64_t n, int64_t env_base,
                                                             uint64_t seed, uint32_t t, int32_t P,
                                                             int32_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * kBlock) {
        const U4 o = draw(env_key(seed, env_base + i), t, kSlotAction);
        const int32_t c = uniform_int(o.v[0], 100);
        int32_t a;
        if (c < 90) a = (int32_t)(o.v[1] & 3u);
        else if (c < 95) a = 4 + P + 1 + uniform_int(o.v[1], 20);
        else if (c < 98) a = 4 + P + 50 + 1 + uniform_int(o.v[1], 20);
        else a = 4 + uniform_int(o.v[2], (uint32_t)P);
        out[i] = a;
    }
}
