// Host-only check of what the state-only step of a fused se_step_seq (step_seq.h,
// step_group_state) reads from step_lean.h and philox.h in place of the forms it had:
//   lean_fuel_scale(w, fifth)  ==  1.0 + (-0.1 + (double)w * fifth), bit for bit, for every one of
//       the 2^32 FUEL words (on at most 16 threads);
//   lean_do_move_val(act - 4, lean_move_bound(P), nodest, inb)  ==  lean_do_move(act, P, nodest, inb)
//       for every action in [-70, 330] and at the int32 ends, P in {0, 1, 5, 64, 254}, every
//       nodest / inb;
//   draw_sched / draw_fuel_sched / draw_gate_pooled_sched under key_schedule(k0, k1)  ==  draw(k, t, slot)
//       for the slots FUEL, GATE, LOSS_0 .. LOSS_3 and ARRIVE, word for word: random and edge keys,
//       quad ids with e1 != 0, counters at both ends of 2^32 and sums that wrap it; the GateSeed
//       travels through a plain row of four words as it does through LDS;
//   gate_window_log2(m): W = 2^log2 is a power of two in [4, 8] with m W <= 64 and 2 m W > 64 or
//       W = 8, for every m in 1 .. 16.
//
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -pthread -o step_trim_check tools/step_trim_check.cpp
//   ./step_trim_check   (prints the numbers of cases; exit status 1 on a mismatch)
//
// tests/test_step_trim_host.py builds and runs it (no GPU needed).
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../shippingenv_amd/csrc/philox.h"
#include "../shippingenv_amd/csrc/step_lean.h"

using namespace shipenv;

static const double kFifthPerWord = 0x1.999999999999ap-35;  // env_core.h: fl(0.2) * 2^-32

static uint64_t bits(double d) {
    uint64_t u;
    std::memcpy(&u, &d, sizeof u);
    return u;
}

// the scale as step_group_state had it: three roundings (the build contracts nothing)
static double scale_former(uint32_t w) { return 1.0 + (-0.1 + (double)w * kFifthPerWord); }

static bool same(const U4& a, const U4& b) { return std::memcmp(a.v, b.v, sizeof a.v) == 0; }

static Key key_of(uint64_t seed, uint64_t quad) {
    Key k;
    k.k0 = (uint32_t)seed;
    k.k1 = (uint32_t)(seed >> 32);
    k.e0 = (uint32_t)quad;
    k.e1 = (uint32_t)(quad >> 32);
    return k;
}

int main() {
    // ---- fuel: all 2^32 words
    unsigned nthreads = std::thread::hardware_concurrency();
    nthreads = nthreads == 0 ? 1 : nthreads > 16 ? 16 : nthreads;
    std::atomic<uint64_t> fuel_bad{0}, first_bad{~0ull};
    std::vector<std::thread> pool;
    const uint64_t total = 1ull << 32, chunk = (total + nthreads - 1) / nthreads;
    for (unsigned i = 0; i < nthreads; ++i)
        pool.emplace_back([&, i] {
            const uint64_t lo = i * chunk, hi = lo + chunk < total ? lo + chunk : total;
            uint64_t bad = 0;
            for (uint64_t w = lo; w < hi; ++w)
                if (bits(scale_former((uint32_t)w)) != bits(lean_fuel_scale((uint32_t)w, kFifthPerWord))) {
                    if (bad++ == 0) {
                        uint64_t cur = first_bad.load();
                        while (w < cur && !first_bad.compare_exchange_weak(cur, w)) {
                        }
                    }
                }
            fuel_bad += bad;
        });
    for (auto& th : pool) th.join();
    if (fuel_bad != 0) {
        const uint32_t w = (uint32_t)first_bad.load();
        std::printf("fuel scale differs for %llu words, first %08x: former %016llx fma %016llx\n", (unsigned long long)fuel_bad.load(),
                    w, (unsigned long long)bits(scale_former(w)), (unsigned long long)bits(lean_fuel_scale(w, kFifthPerWord)));
        return 1;
    }
    // ---- the move test
    std::vector<int> acts;
    for (int a = -70; a <= 330; ++a) acts.push_back(a);
    const int32_t lo = INT32_MIN, hi = INT32_MAX;
    for (int d = 0; d < 8; ++d) {
        acts.push_back(lo + d);
        acts.push_back(hi - d);
    }
    long dec_cases = 0, dec_moves = 0;
    for (int P : {0, 1, 5, 64, 254}) {
        const uint32_t bound = lean_move_bound(P);
        for (int act : acts)
            for (int c = 0; c < 4; ++c) {
                const bool nodest = c & 1, inb = c & 2;
                const int val = (int)((uint32_t)act - 4u);
                const bool want = lean_do_move(act, P, nodest, inb), got = lean_do_move_val(val, bound, nodest, inb);
                ++dec_cases;
                dec_moves += got;
                if (want != got) {
                    std::printf("move test differs: act %d P %d nodest %d inb %d: former %d, on val %d\n", act, P, nodest, inb, want, got);
                    return 1;
                }
            }
    }
    // ---- the scheduled draws
    uint64_t x = 0x2545f4914f6cdd1dull;  // xorshift64*
    auto next = [&x] {
        x ^= x >> 12;
        x ^= x << 25;
        x ^= x >> 27;
        return x * 0x2545f4914f6cdd1dull;
    };
    const uint32_t slots[] = {kSlotFuel, kSlotGate, loss_slot(0), loss_slot(1), loss_slot(2), loss_slot(3), kSlotArrive};
    long draws = 0, e1_nonzero = 0, wrapped = 0, past = 0;
    auto check = [&](uint64_t seed, uint64_t quad, uint32_t t, uint32_t off) {
        const Key k = key_of(seed, quad);
        const KeySched ks = key_schedule(k.k0, k.k1);
        const PairInv inv = pair_invariants(k);
        const GateSeed g = gate_seed(k, inv);
        const uint32_t row[4] = {g.c3, g.hi, g.lo, g.e1};  // the LDS row
        const uint32_t tc = t + off;                       // wraps as the kernel's counter does
        e1_nonzero += k.e1 != 0;
        wrapped += tc < t;
        past += tc < 0x80000000u;
        for (uint32_t slot : slots) {
            ++draws;
            const U4 want = draw(k, tc, slot);
            bool ok = same(draw_sched(ks, k, tc, slot), want);
            if (slot == kSlotFuel) ok &= same(draw_fuel_sched(ks, k, inv, tc), want);
            if (slot == kSlotGate) ok &= same(draw_gate_pooled_sched(ks, GateSeed{row[0], row[1], row[2], row[3]}, tc), want);
            if (!ok) {
                std::printf("scheduled draw differs: seed %016llx quad %016llx t %08x offset %u slot %u\n", (unsigned long long)seed,
                            (unsigned long long)quad, t, off, slot);
                return false;
            }
        }
        return true;
    };
    const uint64_t seeds[] = {0ull, 22ull, 0xffffffffull, 1ull << 32, 0x9e3779b97f4a7c15ull, ~0ull};
    const uint64_t quads[] = {0ull, 1ull, 255ull, 0xffffffffull, 1ull << 32, (1ull << 32) + 7, 1ull << 40, 0x0123456789abcdefull, ~0ull >> 2};
    // counters below 2^32 and just past it (wrapped to 0 ..), and window starts whose offsets wrap
    const uint32_t ts[] = {0u, 1u, 15u, 1000u, 0x7fffffffu, 0x80000000u, 0xfffffff0u, 0xfffffff1u, 0xfffffffdu, 0xffffffffu};
    for (uint64_t s : seeds)
        for (uint64_t q : quads)
            for (uint32_t t : ts)
                for (uint32_t off = 0; off < 16; ++off)
                    if (!check(s, q, t, off)) return 1;
    for (int i = 0; i < 20000; ++i) {
        const uint64_t s = (i & 1) ? next() : (uint32_t)next(), q = (i & 2) ? next() : (uint32_t)next();
        if (!check(s, q, (uint32_t)next(), (uint32_t)next() & 15u)) return 1;
    }
    // ---- the window
    for (uint32_t m = 1; m <= 16; ++m) {
        const uint32_t lg = gate_window_log2(m), W = 1u << lg;
        const bool largest = W == 8 || 2 * m * W > 64;
        if (W < 4 || W > 8 || m * W > 64 || !largest) {
            std::printf("window: m %u gives W %u\n", m, W);
            return 1;
        }
    }
    if (gate_window_log2(1) != 3 || gate_window_log2(8) != 3 || gate_window_log2(9) != 2 || gate_window_log2(16) != 2) {
        std::printf("window: the steps at m = 8, 16 are not where they belong\n");
        return 1;
    }
    if (dec_moves < 32 || e1_nonzero < 1000 || wrapped < 100 || past < 1000) {
        std::printf("coverage: %ld passed moves, %ld tuples with e1 != 0, %ld wrapped, %ld below 2^31\n", dec_moves, e1_nonzero, wrapped, past);
        return 1;
    }
    std::printf("step_trim_check: %llu fuel words on %u threads, %ld move cases (%ld moves), %ld draws (%ld tuples with e1 != 0, %ld with "
                "t + offset past 2^32), 16 windows, new == former\n",
                (unsigned long long)total, nthreads, dec_cases, dec_moves, draws, e1_nonzero, wrapped);
    return 0;
}
