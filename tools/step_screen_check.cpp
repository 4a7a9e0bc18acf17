// Host-only check of the screened GATE pool's helpers (step_lean.h: gate_thr_entry, screen_hot,
// screen_fold; step_seq.h, "The screen").
//   The fold: screen_fold(ballot, log2 W) against the per-offset OR of the ballot's groups of W
//   lanes, W in {4, 8}, in bits 0 .. W - 1: every single-bit ballot, all-ones, zero and 10^5 random
//   ballots.
//   The thresholds: gate_thr_entry, which builds the world image's table, is 0 at cargo 0, all-ones
//   at 50 and never falls over 0 .. 50.
//   The screen is conservative: waves of 1 .. 16 carrier lanes with the kernel's window (W = 8 up
//   to 8 lanes, 4 above), each lane's four cargos drawn from [-3, 60] (the thresholds at the vote:
//   the entry of the cargo clamped to 0 .. 50), cargo paths that only fall from step to step (to
//   zero or below too; every other window holds cargo up to 3 only), random words and the edges
//   (0, all-ones, the threshold at the vote, one above it, the current threshold). The lane of
//   carrier c and offset s screens its block as the refill does; the ballot is folded; and wherever the exact test `cargo > 0 && word <=
//   threshold of the cargo now` fires at offset s, bit s of the fold is set. It also counts the
//   clear bits and the fires after a fall, so that the check cannot pass by a screen that is
//   always set.
//
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -o step_screen_check tools/step_screen_check.cpp
//   ./step_screen_check   (prints the numbers of cases; exit status 1 on a mismatch)
// It may be built with -Xarch_host -fsanitize=address,undefined as its own program.
//
// tests/test_step_screen_host.py builds and runs it (no GPU needed).
#include <cstdio>
#include <vector>

#include "../shippingenv_amd/csrc/step_lean.h"

using namespace shipenv;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static uint32_t fold_brute(uint64_t ballot, uint32_t logw) {
    const uint32_t W = 1u << logw;
    uint32_t out = 0;
    for (uint32_t L = 0; L < 64; ++L)
        if ((ballot >> L) & 1u) out |= 1u << (L & (W - 1u));
    return out;
}

static uint32_t thr_of(int cargo) { return gate_thr_entry(cargo < 0 ? 0 : cargo > 50 ? 50 : cargo, 50.0); }

int main() {
    // ---- the fold
    long folds = 0;
    for (uint32_t logw : {2u, 3u}) {
        std::vector<uint64_t> ballots = {0ull, ~0ull};
        for (int b = 0; b < 64; ++b) ballots.push_back(1ull << b);
        for (int i = 0; i < 100000; ++i) ballots.push_back(i % 3 == 0 ? rnd() & rnd() & rnd() : rnd());
        for (uint64_t b : ballots) {
            ++folds;
            if ((screen_fold(b, logw) & ((1u << (1u << logw)) - 1u)) != fold_brute(b, logw)) {  // bits 0 .. W - 1 are the fold's
                std::printf("fold: ballot %016llx W %u: %x, not %x\n", (unsigned long long)b, 1u << logw, screen_fold(b, logw),
                            fold_brute(b, logw));
                return 1;
            }
        }
    }
    // ---- the thresholds of the image
    if (gate_thr_entry(0, 50.0) != 0u || gate_thr_entry(50, 50.0) != 0xffffffffu || gate_thr_entry(25, 50.0) != 0x80000000u) {
        std::printf("gate_thr_entry: ends %x %x, middle %x\n", gate_thr_entry(0, 50.0), gate_thr_entry(50, 50.0), gate_thr_entry(25, 50.0));
        return 1;
    }
    for (int c = 1; c <= 50; ++c)
        if (gate_thr_entry(c, 50.0) < gate_thr_entry(c - 1, 50.0)) {
            std::printf("gate_thr_entry falls at cargo %d\n", c);
            return 1;
        }
    // ---- the screen is conservative
    long windows = 0, fires = 0, fires_after_fall = 0, clear_bits = 0, set_bits = 0, edge_words = 0;
    for (int it = 0; it < 20000; ++it) {
        const uint32_t m = 1u + (uint32_t)(rnd() % 16), logw = gate_window_log2(m), W = 1u << logw;
        int vote[16][4];
        uint32_t thr0[16][4];
        for (uint32_t c = 0; c < m; ++c) {
            bool any = false;
            for (int j = 0; j < 4; ++j) {
                const uint64_t r = rnd();
                // every other window holds light ships only (cargo up to 3: most of its steps are cold)
                vote[c][j] = it % 2 ? (int)((r >> 8) % 7) - 3
                                    : r % 5 == 0 ? 50 + (int)(r >> 8) % 11 : r % 5 == 1 ? -(int)((r >> 8) % 4) : (int)((r >> 8) % 61) - 3;
                any |= vote[c][j] > 0;
            }
            if (!any) vote[c][(int)(rnd() % 4)] = 1 + (int)(rnd() % (it % 2 ? 3 : 59));  // a carrier lane holds cargo
            for (int j = 0; j < 4; ++j) thr0[c][j] = thr_of(vote[c][j]);
        }
        // cargo[s][c][j] before step s: it only falls
        std::vector<int> cargo((size_t)W * 16 * 4);
        for (uint32_t c = 0; c < m; ++c)
            for (int j = 0; j < 4; ++j) {
                int cur = vote[c][j];
                for (uint32_t s = 0; s < W; ++s) {
                    cargo[(s * 16 + c) * 4 + j] = cur;
                    const uint64_t r = rnd();
                    if (r % 3 == 0 && cur > 0) cur -= (int)((r >> 8) % (uint64_t)(cur + 1));  // a partial or whole loss
                    else if (r % 17 == 0) cur = 0;                                                // an arrival
                }
            }
        // the words of carrier c at offset s
        std::vector<uint32_t> word((size_t)W * 16 * 4);
        for (uint32_t c = 0; c < m; ++c)
            for (uint32_t s = 0; s < W; ++s)
                for (int j = 0; j < 4; ++j) {
                    const uint64_t r = rnd();
                    const uint32_t now = thr_of(cargo[(s * 16 + c) * 4 + j]);
                    uint32_t v = (uint32_t)(r >> 32);
                    switch (r % 64) {
                        case 0: v = 0u; break;
                        case 1: v = 0xffffffffu; break;
                        case 2: v = thr0[c][j]; break;
                        case 3: v = thr0[c][j] + 1u; break;  // wraps to 0 at all-ones
                        case 4: v = now; break;
                        case 5: v = now + 1u; break;
                        case 6: v = (uint32_t)(((uint64_t)(now) * (r >> 40)) >> 24); break;  // at or below the threshold now
                        default: break;
                    }
                    edge_words += r % 64 < 6;
                    word[(s * 16 + c) * 4 + j] = v;
                }
        // the refill: lane L screens carrier min(L >> logw, m - 1)'s block at offset L & (W - 1)
        uint64_t ballot = 0;
        for (uint32_t L = 0; L < 64; ++L) {
            const uint32_t c = (L >> logw) < m - 1u ? (L >> logw) : m - 1u, s = L & (W - 1u);
            if (screen_hot(&word[(s * 16 + c) * 4], thr0[c])) ballot |= 1ull << L;
        }
        const uint32_t screen = screen_fold(ballot, logw);
        ++windows;
        for (uint32_t s = 0; s < W; ++s) {
            const bool bit = (screen >> s) & 1u;
            set_bits += bit;
            clear_bits += !bit;
            for (uint32_t c = 0; c < m; ++c)
                for (int j = 0; j < 4; ++j) {
                    const int cg = cargo[(s * 16 + c) * 4 + j];
                    const bool fire = cg > 0 && word[(s * 16 + c) * 4 + j] <= thr_of(cg);
                    fires += fire;
                    fires_after_fall += fire && cg < vote[c][j];
                    if (fire && !bit) {
                        std::printf("screen: m %u W %u carrier %u env %d offset %u: cargo %d (at the vote %d) word %08x fires on a cold step\n",
                                    m, W, c, j, s, cg, vote[c][j], word[(s * 16 + c) * 4 + j]);
                        return 1;
                    }
                }
        }
    }
    if (fires < 10000 || fires_after_fall < 1000 || clear_bits < 1000 || set_bits < 1000 || edge_words < 10000) {
        std::printf("coverage: %ld fires, %ld after a fall, %ld clear bits, %ld set bits, %ld edge words\n", fires, fires_after_fall,
                    clear_bits, set_bits, edge_words);
        return 1;
    }
    std::printf("step_screen_check: %ld folds, 51 thresholds, %ld windows (%ld fires, %ld after a fall, %ld clear bits, %ld set bits), "
                "fold == OR, every fire on a hot step\n", folds, windows, fires, fires_after_fall, clear_bits, set_bits);
    return 0;
}
