// Host-only check of the GATE pool's windows sized to the carriers and of the arrival test by the
// cell code (step_lean.h: gate_window_entry, gate_lane_offset / _carrier, gate_pool_index,
// gate_screen_mask / _step, ports_on_distinct_cells, arrive_by_code; step_seq.h, "The wave's GATE
// pool" and step_group_ring).
//   Windows, for every m in 1 .. 16: W = min(16, 64 / m) is 4 .. 16 with m W <= 64; lane L -> (L - s m,
//   s = L / m by the reciprocal multiply) is a bijection from the lanes below m W onto (carrier,
//   offset) and gives every other lane a carrier below m and an offset >= W; the entry any lane can
//   read (a carrier at its rank, a non-carrier at a rank up to m, every offset of the window) lies
//   inside the wave's kGatePoolRow rows, a carrier's below 64 and at the lane that drew its block.
//   The screen: the ballot shifted down by m per step and tested against its low m bits equals the
//   per-offset OR of the ballot's bits, for every m: zero, all-ones, every single bit and 10^5 random
//   ballots; m == 0 tests the launch's screen_all alone.
//   Monotonicity: windows of every m, each lane's four thresholds taken at the vote, cargo paths
//   that only fall (a loss, an arrival), and in mid-window takes of fuel and refused takes, which
//   leave cargo as it is and whose env does not move in that step; random words and the edges. Every
//   step on which the exact gate test fires has its screen bit set. It fails if the count of fires, of
//   fires after a fall, of fires after a take that left the window standing or of clear bits is 0.
//   Arrival: maps of 1 x 1, 1 x 7, 5 x 9 and 100 x 100 cells with P in {1, 5, 253} ports on distinct
//   cells (where the map has that many), some ground; a ship on every cell, every dest < P, do_move
//   both ways: the test by the code equals the position compare. ports_on_distinct_cells is true
//   for these worlds and false as soon as two ports share a cell; the launch's bit
//   (arrive_by_code_allowed) also asks for at least two ports.
//
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -o step_window_check tools/step_window_check.cpp
//   ./step_window_check   (prints the numbers of cases; exit status 1 on a mismatch)
// It may be built with -Xarch_host -fsanitize=address,undefined as its own program.
//
// tests/test_step_window_host.py builds and runs it (no GPU needed).
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

static uint32_t thr_of(int cargo) { return gate_thr_entry(cargo < 0 ? 0 : cargo > 50 ? 50 : cargo, 50.0); }

// bit s of the result: some lane L < 64 with L / m == s has its ballot bit set
static uint32_t screen_brute(uint64_t ballot, uint32_t m, uint32_t W) {
    uint32_t out = 0;
    for (uint32_t L = 0; L < 64; ++L)
        if (((ballot >> L) & 1u) && L / m < W) out |= 1u << (L / m);
    return out;
}
// the window's walk, as step_seq_kernel runs it
static uint32_t screen_walk(uint64_t ballot, uint32_t m, uint32_t W) {
    const uint64_t mask = gate_screen_mask(m);
    uint32_t out = 0;
    for (uint32_t s = 0; s < W; ++s) {
        if (gate_screen_step(ballot, mask)) out |= 1u << s;
        ballot >>= m;
    }
    return out;
}

int main() {
    static_assert(gate_pool_reads_in_rows(), "the bound the library checks at compile time");
    // ---- the windows and the lane mapping
    long lanes = 0, reads = 0;
    for (uint32_t m = 1; m <= kGatePoolLimit; ++m) {
        const uint32_t e = gate_window_entry(m), W = gate_window_len(e);
        const uint32_t want = 64u / m < 16u ? 64u / m : 16u;
        if (e != gate_window_entry_of(m) || W != want || W < 4 || W > 16 || m * W > 64) {
            std::printf("window: m %u W %u (min(16, 64 / m) is %u)\n", m, W, want);
            return 1;
        }
        std::vector<int> seen((size_t)m * W, 0);
        for (uint32_t L = 0; L < 64; ++L) {
            const uint32_t s = gate_lane_offset(L, e), c = gate_lane_carrier(L, s, m);
            ++lanes;
            if (s != L / m || c != L % m) {
                std::printf("mapping: m %u lane %u -> offset %u carrier %u, not %u %u\n", m, L, s, c, L / m, L % m);
                return 1;
            }
            if (L < m * W) {
                if (s >= W || c >= m || seen[(size_t)s * m + c]++) {
                    std::printf("mapping: m %u lane %u -> (%u, %u) twice or outside the window\n", m, L, c, s);
                    return 1;
                }
                if (gate_pool_index(s, m, c) != L) {  // the carrier of rank c reads at offset s what lane L drew
                    std::printf("mapping: m %u carrier %u offset %u reads entry %u, lane %u drew it\n", m, c, s, gate_pool_index(s, m, c), L);
                    return 1;
                }
            } else if (s < W || c >= m) {
                std::printf("mapping: m %u lane %u past the window -> (%u, %u)\n", m, L, c, s);
                return 1;
            }
        }
        for (int v : seen)
            if (v != 1) {
                std::printf("mapping: m %u: a (carrier, offset) no lane draws\n", m);
                return 1;
            }
        // every read: a lane's rank is the number of carrier lanes below it, 0 .. m (m: a non-carrier above all)
        for (uint32_t slot = 0; slot <= m; ++slot)
            for (uint32_t s = 0; s < W; ++s) {
                const uint32_t i = gate_pool_index(s, m, slot);
                ++reads;
                if (i >= kGatePoolRow || (slot < m && i >= 64)) {
                    std::printf("read: m %u rank %u offset %u reads entry %u\n", m, slot, s, i);
                    return 1;
                }
            }
    }
    if (gate_window_len(gate_window_entry(0)) != 16 || gate_pool_index(1000000u, 0, 0) != 0) {
        std::printf("window: m 0\n");
        return 1;
    }
    // ---- the screen's walk
    long walks = 0;
    for (uint32_t m = 1; m <= kGatePoolLimit; ++m) {
        const uint32_t W = gate_window_len(gate_window_entry(m));
        std::vector<uint64_t> ballots = {0ull, ~0ull};
        for (int b = 0; b < 64; ++b) ballots.push_back(1ull << b);
        for (int i = 0; i < 100000; ++i) ballots.push_back(i % 3 == 0 ? rnd() & rnd() & rnd() : rnd());
        for (uint64_t b : ballots) {
            ++walks;
            if (screen_walk(b, m, W) != screen_brute(b, m, W)) {
                std::printf("screen: ballot %016llx m %u W %u: %x, not %x\n", (unsigned long long)b, m, W, screen_walk(b, m, W), screen_brute(b, m, W));
                return 1;
            }
        }
    }
    // m == 0: the launch's screen_all alone (0: every step cold, all-ones: every step hot), however long the window
    if (screen_walk(0ull, 0, 32) != 0u || screen_walk(~0ull, 0, 32) != 0xffffffffu) {
        std::printf("screen: m 0\n");
        return 1;
    }
    // ---- the screen is conservative under the new ending rule
    long windows = 0, fires = 0, fires_after_fall = 0, fires_after_kept_take = 0, clear_bits = 0, set_bits = 0, edge_words = 0;
    for (int it = 0; it < 32000; ++it) {
        const uint32_t m = 1u + (uint32_t)(it % 16), e = gate_window_entry(m), W = gate_window_len(e);
        int vote[16][4];
        uint32_t thr0[16][4];
        for (uint32_t c = 0; c < m; ++c) {
            bool any = false;
            for (int j = 0; j < 4; ++j) {
                const uint64_t r = rnd();
                // every other round of the 16 window lengths holds light ships only (most of its steps are cold)
                vote[c][j] = (it / 16) % 2 ? (int)((r >> 8) % 7) - 3
                                           : r % 5 == 0 ? 50 + (int)(r >> 8) % 11 : r % 5 == 1 ? -(int)((r >> 8) % 4) : (int)((r >> 8) % 61) - 3;
                any |= vote[c][j] > 0;
            }
            if (!any) vote[c][(int)(rnd() % 4)] = 1 + (int)(rnd() % ((it / 16) % 2 ? 3 : 59));  // a carrier lane holds cargo
            for (int j = 0; j < 4; ++j) thr0[c][j] = thr_of(vote[c][j]);
        }
        // cargo[s][c][j] before step s: it only falls. stays[s][c][j]: the env takes fuel or is refused a
        // take in step s (its take block runs, the window stands, the env does not move: no gate).
        std::vector<int> cargo((size_t)W * 16 * 4), stays((size_t)W * 16 * 4, 0), kept((size_t)W * 16 * 4, 0);
        for (uint32_t c = 0; c < m; ++c)
            for (int j = 0; j < 4; ++j) {
                int cur = vote[c][j], took = 0;
                for (uint32_t s = 0; s < W; ++s) {
                    const size_t i = (s * 16 + c) * 4 + j;
                    cargo[i] = cur;
                    kept[i] = took;
                    const uint64_t r = rnd();
                    if (r % 11 == 0) stays[i] = took = 1;                                            // a take of fuel, a refused take
                    else if (r % 3 == 0 && cur > 0) cur -= (int)((r >> 8) % (uint64_t)(cur + 1));  // a partial or whole loss
                    else if (r % 17 == 0) cur = 0;                                                  // an arrival
                }
            }
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
        // the refill: lane L screens carrier L - s m's block at offset s = L / m; past the window: words nobody reads
        uint64_t ballot = 0;
        for (uint32_t L = 0; L < 64; ++L) {
            const uint32_t s = gate_lane_offset(L, e), c = gate_lane_carrier(L, s, m);
            uint32_t junk[4] = {(uint32_t)rnd(), 0u, (uint32_t)rnd(), 0xffffffffu};
            if (screen_hot(s < W ? &word[(s * 16 + c) * 4] : junk, thr0[c])) ballot |= 1ull << L;
        }
        const uint64_t mask = gate_screen_mask(m);
        ++windows;
        for (uint32_t s = 0; s < W; ++s) {
            const bool bit = gate_screen_step(ballot, mask);
            ballot >>= m;
            set_bits += bit;
            clear_bits += !bit;
            for (uint32_t c = 0; c < m; ++c)
                for (int j = 0; j < 4; ++j) {
                    const size_t i = (s * 16 + c) * 4 + j;
                    const int cg = cargo[i];
                    const bool fire = !stays[i] && cg > 0 && word[i] <= thr_of(cg);
                    fires += fire;
                    fires_after_fall += fire && cg < vote[c][j];
                    fires_after_kept_take += fire && kept[i];
                    if (fire && !bit) {
                        std::printf("screen: m %u W %u carrier %u env %d offset %u: cargo %d (at the vote %d) word %08x fires on a cold step\n",
                                    m, W, c, j, s, cg, vote[c][j], word[i]);
                        return 1;
                    }
                }
        }
    }
    if (fires == 0 || fires_after_fall == 0 || fires_after_kept_take == 0 || clear_bits == 0 || set_bits == 0 || edge_words == 0) {
        std::printf("coverage: %ld fires, %ld after a fall, %ld after a kept take, %ld clear bits, %ld set bits, %ld edge words\n", fires,
                    fires_after_fall, fires_after_kept_take, clear_bits, set_bits, edge_words);
        return 1;
    }
    // ---- the arrival test by the cell code
    long arrivals = 0, tests = 0, worlds = 0;
    const int maps[4][2] = {{1, 1}, {1, 7}, {5, 9}, {100, 100}};
    for (const auto& hw : maps) {
        const int H = hw[0], W = hw[1];
        for (int P : {1, 5, 253}) {
            if (P > H * W) continue;
            ++worlds;
            // P distinct cells, a fifth of the others ground
            std::vector<int> cells((size_t)H * W);
            for (int i = 0; i < H * W; ++i) cells[(size_t)i] = i;
            for (int i = H * W - 1; i > 0; --i) std::swap(cells[(size_t)i], cells[(size_t)(rnd() % (uint64_t)(i + 1))]);
            std::vector<int32_t> px((size_t)P), py((size_t)P);
            std::vector<uint8_t> code((size_t)H * W, 0);
            for (int i = P; i < H * W; ++i)
                if (rnd() % 5 == 0) code[(size_t)cells[(size_t)i]] = (uint8_t)kRingGround;
            for (int i = P - 1; i >= 0; --i) {  // the world image's stamps: the first port on a cell wins
                px[(size_t)i] = cells[(size_t)i] / W;
                py[(size_t)i] = cells[(size_t)i] % W;
                code[(size_t)cells[(size_t)i]] = (uint8_t)(i + 1);
            }
            if (!ports_on_distinct_cells(P, px.data(), py.data())) {
                std::printf("distinct: %d x %d, %d ports on distinct cells called shared\n", H, W, P);
                return 1;
            }
            for (int x = 0; x < H; ++x)
                for (int y = 0; y < W; ++y)
                    for (int dst = 0; dst < P; ++dst)
                        for (int mv = 0; mv < 2; ++mv) {
                            const bool by_pos = (mv != 0) & (x == px[(size_t)dst] && y == py[(size_t)dst]);
                            const bool by_code = arrive_by_code(mv != 0, code[(size_t)x * W + y], dst);
                            ++tests;
                            arrivals += by_pos;
                            if (by_pos != by_code) {
                                std::printf("arrival: %d x %d P %d ship (%d, %d) dest %d do_move %d: by code %d, by position %d\n", H, W, P, x, y,
                                            dst, mv, by_code, by_pos);
                                return 1;
                            }
                        }
            // two ports on one cell: every pair of a few, the others left apart
            for (int a = 0; a < P && a < 6; ++a)
                for (int b = 0; b < P; ++b) {
                    if (a == b) continue;
                    std::vector<int32_t> qx = px, qy = py;
                    qx[(size_t)b] = px[(size_t)a];
                    qy[(size_t)b] = py[(size_t)a];
                    if (ports_on_distinct_cells(P, qx.data(), qy.data())) {
                        std::printf("distinct: %d x %d, ports %d and %d on one cell called distinct\n", H, W, a, b);
                        return 1;
                    }
                }
        }
    }
    // the launch's bit: never with fewer than two ports (an arrival in a world of one port leaves dest == P), never with a shared cell
    if (arrive_by_code_allowed(0, true) || arrive_by_code_allowed(1, true) || !arrive_by_code_allowed(2, true) ||
        !arrive_by_code_allowed(253, true) || arrive_by_code_allowed(2, false) || arrive_by_code_allowed(5, false)) {
        std::printf("arrival: the launch's bit for P in {0, 1, 2, 253}\n");
        return 1;
    }
    if (!ports_on_distinct_cells(0, nullptr, nullptr) || worlds != 8 || arrivals == 0) {
        std::printf("arrival: %ld worlds, %ld arrivals\n", worlds, arrivals);
        return 1;
    }
    std::printf("step_window_check: %ld lanes, %ld reads, %ld walks, %ld windows (%ld fires, %ld after a fall, %ld after a kept take, "
                "%ld clear bits, %ld set bits), %ld worlds (%ld arrival tests, %ld arrivals): mapping a bijection, reads in rows, "
                "walk == OR, every fire on a hot step, by code == by position\n",
                lanes, reads, walks, windows, fires, fires_after_fall, fires_after_kept_take, clear_bits, set_bits, worlds, tests, arrivals);
    return 0;
}
