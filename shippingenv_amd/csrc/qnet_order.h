#pragma once
// qnet_order.h — the policy kernels' visiting order: OrderRun (load, count, place), kOrderNone
// and kOrderScanBytes.
//
// A fragment of shipenv.hip's translation unit, included inside qpolicy.h's anonymous
// namespace before the policy kernels: not a stand-alone header. Uses world.h (LdsWorld).

// ------------------------------------------------------------------ visiting order
// Only a ship on a port's cell can take anything but the 4 moves (is_valid_action,
// agents/dqn.py:125-175): its valid rows reach fc3's second 32-row tile (the TAKE_FUEL
// amounts), while a ship at sea needs rows 0-3 of tile 0. The policy kernels skip a
// tile no env of the wave can use, but with ~1 ship in 5 in port hardly a 32-env tile
// is all at sea (0.8^32). So from 2^16 envs each workgroup takes a contiguous chunk of envs
// and first lists them in an order where they are: its ships at sea first, then those in
// port, each group in ascending env order (order_chunk, written to a scratch list the
// workgroup alone reads); its waves then take the chunk's 32-env tiles round robin, so
// ~3 in 4 of the tiles skip fc3's second tile and every wave meets its share of in-port
// tiles. The order changes only which lane computes which env: every output is keyed by the
// env (actions, Philox draws, replay slots), so results are identical to position order.
// (Round 6 first built the order in a kernel of its own: 5.6 us per call in the trace.)
// In two halves, so that a kernel can stage its image between them (the counting half's
// loads then overlap the staging): count() walks thread t's own run [b, e) of the chunk and
// counts its ships in port; place() scans the counts over the workgroup (wsum: kBlock / 64 u64
// of LDS) and writes the list. place() ends with a barrier.
constexpr uint32_t kOrderNone = 0xffffffffu;
struct OrderRun {
    int b = 0, e = 0;
    uint32_t port = 0u, bits = 0u;  // bits: the first 32 envs' in-port flags, for place()
    // load(): a run of 4, 8, 12 or 16 envs on a 4-byte boundary (2^20 envs: 4 per thread in the
    // bf16 kernel, 8 in the fp32 one) is loaded as whole words, issued before the image is
    // staged and used after it, so the loads overlap the staging; other runs go byte by byte
    // in count() (the first form issued a dependent load chain per env: +3.3 / +8.6 us on the
    // two kernels' prologues, profiles/r06/order/trace_prologue.jsonl)
    static constexpr int kWords = 4;
    uint32_t xw[kWords] = {}, yw[kWords] = {};
    bool words = false;

    template <int kBlock>
    __device__ __forceinline__ void load(const uint8_t* xs, const uint8_t* ys, int64_t c0, int len) {
        const int per = (len + kBlock - 1) / kBlock;
        b = (int)threadIdx.x * per;
        e = min(b + per, len);
        // uniform; with len a multiple of 4 every run is whole words, none reads past the chunk
        words = (per & 3) == 0 && per <= 4 * kWords && (c0 & 3) == 0 && (len & 3) == 0;
        if (words) {
            const uint32_t* x4 = reinterpret_cast<const uint32_t*>(xs + c0 + b);
            const uint32_t* y4 = reinterpret_cast<const uint32_t*>(ys + c0 + b);
#pragma unroll
            for (int k = 0; k < kWords; ++k) {
                if (4 * k < e - b) {  // e - b: per, or a shorter multiple of 4 for the chunk's last runs
                    xw[k] = x4[k];
                    yw[k] = y4[k];
                }
            }
        }
    }

    template <int kBlock>
    __device__ __forceinline__ void count(const LdsWorld& w, const uint8_t* xs, const uint8_t* ys, int64_t c0) {
        if (words) {
#pragma unroll
            for (int k = 0; k < 4 * kWords; ++k) {
                if (k < e - b) {
                    const int x = (int)((xw[k >> 2] >> (8 * (k & 3))) & 0xffu), y = (int)((yw[k >> 2] >> (8 * (k & 3))) & 0xffu);
                    const uint32_t f = w.port_at(x, y) >= 0 ? 1u : 0u;
                    port += f;
                    bits |= f << k;
                }
            }
            return;
        }
        for (int i = b; i < e; ++i) {
            const uint32_t f = w.port_at(xs[c0 + i], ys[c0 + i]) >= 0 ? 1u : 0u;
            port += f;
            bits |= i - b < 32 ? f << (i - b) : 0u;
        }
    }

    // the list's tail up to a whole tile reads all ones (an idle lane). T = uint32_t: the envs
    // (a global scratch list); T = uint16_t: their indices in the chunk (an LDS list)
    template <int kBlock, typename T>
    __device__ __forceinline__ void place(const LdsWorld& w, const uint8_t* xs, const uint8_t* ys, int64_t c0,
                                          int len, T* out, uint64_t* wsum) const {
        constexpr bool kLocal = sizeof(T) == 2;
        if ((int)threadIdx.x < ((-len) & 31)) out[len + threadIdx.x] = (T)~(T)0;
        const uint32_t sea = (uint32_t)max(e - b, 0) - port;
        // exclusive prefix of (at sea, in port) over the threads, as two 32-bit halves
        const uint64_t mine = (uint64_t)sea | (uint64_t)port << 32;
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        uint64_t inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t u = __shfl_up(inc, d);
            inc += lane >= d ? u : 0ull;
        }
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        uint64_t off = 0ull, total = 0ull;
#pragma unroll
        for (int i = 0; i < kBlock / 64; ++i) {
            off += i < wv ? wsum[i] : 0ull;
            total += wsum[i];
        }
        const uint64_t ex = inc - mine + off;
        uint32_t at_sea = (uint32_t)ex, in_port = (uint32_t)total + (uint32_t)(ex >> 32);
        for (int i = b; i < e; ++i) {
            const bool p = i - b < 32 ? ((bits >> (i - b)) & 1u) != 0u : w.port_at(xs[c0 + i], ys[c0 + i]) >= 0;
            out[p ? in_port : at_sea] = kLocal ? (T)i : (T)(c0 + i);
            in_port += p ? 1u : 0u;
            at_sea += p ? 0u : 1u;
        }
        __threadfence_block();  // the list is complete before any wave of the workgroup reads it
        __syncthreads();
    }
};
constexpr int kOrderScanBytes = 16 * 8;  // place()'s wsum, past the policy's LDS (<= 16 waves)
