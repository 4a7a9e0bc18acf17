// Host-only check of the regular state-only step's decode on the bordered cell table
// (step_lean.h: ring_table_build, ring_bias / ring_unbias, ring_index, ring_do_move, ring_moved;
// step_seq.h, step_group_ring) against the general form (step_group_state): the bounds test on
// the packed position, the select of the cell to read, the ground test on that cell's code,
// lean_do_move_val and `moved = do_move & !ground`.
//   Maps of H x W in {1 x 1, 1 x 7, 7 x 1, 5 x 9, 100 x 100}, P in {0, 1, 5, 253}; the cells' codes
//   cycle through water, ground, a port's code and a code past P in four phases, so every cell is
//   of every class under the ship and at the target; a ship on every cell; every action in
//   [-70, 330] and at the int32 ends. For each: do_move, moved, the next position (after the bias
//   comes off) and the next carried code are the general form's.
//   The table against the image: the interior is the map, the ring is kRingBorder, the padding
//   zero. ring_unbias(ring_bias(p)) == p for every x, y < 256. ring_table_fits says no for
//   P = 254, for a map whose table leaves no room beside the launch's other LDS, and one byte
//   past the limit; yes for the 100 x 100 map with 20 KiB of other LDS and exactly at the limit.
//
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -o step_ring_check tools/step_ring_check.cpp
//   ./step_ring_check   (prints the numbers of cases; exit status 1 on a mismatch)
// It may be built with -fsanitize=address,undefined as its own program.
//
// tests/test_step_ring_host.py builds and runs it (no GPU needed).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../shippingenv_amd/csrc/step_lean.h"

using namespace shipenv;

static uint32_t pk_add_u16(uint32_t a, uint32_t b) { return ((a + b) & 0xffffu) | ((((a >> 16) + (b >> 16)) & 0xffffu) << 16); }
static uint32_t pk_min_u16(uint32_t a, uint32_t b) {
    const uint32_t lo = (a & 0xffffu) < (b & 0xffffu) ? (a & 0xffffu) : (b & 0xffffu);
    const uint32_t hi = (a >> 16) < (b >> 16) ? (a >> 16) : (b >> 16);
    return lo | (hi << 16);
}

enum Class { kWater, kGround, kPort, kPast, kClasses };

// the code of cell c in a phase, and its class (a class the world cannot hold falls back to water)
static uint8_t code_of(int c, int phase, int P, Class& cls) {
    cls = (Class)((c + phase) & 3);
    if (cls == kPort && P > 0) return (uint8_t)(1 + c % P);
    if (cls == kPast && P + 1 <= 253) return (uint8_t)(P + 1 + c % (253 - P));
    if (cls == kGround) return (uint8_t)kRingGround;
    cls = kWater;
    return 0;
}

int main() {
    // N, E, S, W as packed 16-bit (dx, dy), as the world image holds them
    const int mdx[4] = {0, -1, 0, 1}, mdy[4] = {-1, 0, 1, 0};
    uint32_t moves[4];
    for (int k = 0; k < 4; ++k) moves[k] = ((uint32_t)mdx[k] & 0xffffu) | (((uint32_t)mdy[k] & 0xffffu) << 16);
    std::vector<int> acts;
    for (int a = -70; a <= 330; ++a) acts.push_back(a);
    for (int d = 0; d < 8; ++d) {
        acts.push_back(INT32_MIN + d);
        acts.push_back(INT32_MAX - d);
    }
    const int maps[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 9}, {100, 100}};
    long cases = 0, off_map = 0, blocked = 0, moves_made = 0, tables = 0;
    long under[kClasses] = {0, 0, 0, 0}, target[kClasses] = {0, 0, 0, 0};
    for (const auto& hw : maps) {
        const int H = hw[0], W = hw[1];
        for (int P : {0, 1, 5, 253}) {
            const uint32_t bound = lean_move_bound(P);
            for (int phase = 0; phase < 4; ++phase) {
                std::vector<uint8_t> cell((size_t)H * W);
                std::vector<Class> cls((size_t)H * W);
                for (int c = 0; c < H * W; ++c) cell[c] = code_of(c, phase, P, cls[c]);
                // ---- the table against the image; exactly sized, so a sanitizer sees a stray index
                std::vector<uint8_t> ring(ring_table_bytes(H, W));
                ring_table_build(H, W, cell.data(), ring.data());
                ++tables;
                if (ring.size() % 16 != 0 || ring.size() < (size_t)(H + 2) * (W + 2) || ring.size() >= (size_t)(H + 2) * (W + 2) + 16) {
                    std::printf("table size %zu for %d x %d\n", ring.size(), H, W);
                    return 1;
                }
                for (int bx = 0; bx < H + 2; ++bx)
                    for (int by = 0; by < W + 2; ++by) {
                        const bool inside = bx >= 1 && bx <= H && by >= 1 && by <= W;
                        const uint8_t want = inside ? cell[(size_t)(bx - 1) * W + (by - 1)] : (uint8_t)kRingBorder;
                        const uint8_t got = ring[ring_index((uint32_t)bx | ((uint32_t)by << 16), W)];
                        if (got != want) {
                            std::printf("table %d x %d P %d: (%d, %d) holds %u, not %u\n", H, W, P, bx, by, got, want);
                            return 1;
                        }
                    }
                for (size_t i = (size_t)(H + 2) * (W + 2); i < ring.size(); ++i)
                    if (ring[i] != 0) {
                        std::printf("table %d x %d: padding byte %zu is %u\n", H, W, i, ring[i]);
                        return 1;
                    }
                // ---- the decode
                const uint32_t lim = (uint32_t)(H - 1) | ((uint32_t)(W - 1) << 16);
                for (int x = 0; x < H; ++x)
                    for (int y = 0; y < W; ++y) {
                        const uint32_t p = (uint32_t)x | ((uint32_t)y << 16), bp = ring_bias(p);
                        const uint32_t code = cell[(size_t)x * W + y];
                        for (int act : acts) {
                            const int val = (int)((uint32_t)act - 4u);
                            const uint32_t dxy = moves[act & 3];
                            // the general form (a regular env has a destination)
                            const uint32_t np = pk_add_u16(p, dxy);
                            const bool inb = pk_min_u16(np, lim) == np;
                            const uint32_t cp = inb ? np : p;
                            const uint32_t code_cp = cell[(size_t)(cp & 0xffffu) * W + (cp >> 16)];
                            const bool ground = code_cp == kRingGround;
                            const bool do_move = lean_do_move_val(val, bound, false, inb);
                            const bool moved = do_move & !ground;
                            const uint32_t pos1 = moved ? cp : p, code1 = moved ? code_cp : code;
                            // the regular form
                            const uint32_t nbp = pk_add_u16(bp, dxy);
                            const uint32_t idx = ring_index(nbp, W);
                            if (idx >= (uint32_t)(H + 2) * (uint32_t)(W + 2)) {
                                std::printf("index %u outside the table of %d x %d: (%d, %d) act %d\n", idx, H, W, x, y, act);
                                return 1;
                            }
                            const uint32_t code_t = ring[idx];
                            const bool r_do_move = ring_do_move(val, bound, code_t), r_moved = ring_moved(val, bound, code_t);
                            const uint32_t r_pos1 = ring_unbias(r_moved ? nbp : bp), r_code1 = r_moved ? code_t : code;
                            ++cases;
                            if (do_move != r_do_move || moved != r_moved || pos1 != r_pos1 || code1 != r_code1) {
                                std::printf("%d x %d P %d phase %d (%d, %d) act %d: general do_move %d moved %d pos %08x code %u, "
                                            "regular %d %d %08x %u\n", H, W, P, phase, x, y, act, do_move, moved, pos1, code1, r_do_move,
                                            r_moved, r_pos1, r_code1);
                                return 1;
                            }
                            const bool is_mv = (uint32_t)val > bound;
                            off_map += is_mv && !inb;
                            blocked += do_move && !moved;
                            moves_made += moved;
                            if (is_mv && inb) {
                                ++under[cls[(size_t)x * W + y]];
                                ++target[cls[(size_t)(cp & 0xffffu) * W + (cp >> 16)]];
                            }
                        }
                    }
            }
        }
    }
    // ---- the bias round trip
    long trips = 0;
    for (uint32_t x = 0; x < 256; ++x)
        for (uint32_t y = 0; y < 256; ++y) {
            const uint32_t p = x | (y << 16), bp = ring_bias(p);
            ++trips;
            if ((bp & 0xffffu) != x + 1 || (bp >> 16) != y + 1 || ring_unbias(bp) != p) {
                std::printf("bias: (%u, %u) -> %08x -> %08x\n", x, y, bp, ring_unbias(bp));
                return 1;
            }
        }
    // ---- the choice of a launch with or without the table
    const size_t other = 20 * 1024;  // the 100 x 100 image, the stock table and the GATE pools
    const uint32_t t100 = ring_table_bytes(100, 100);
    const bool fits_ok = ring_table_fits(100, 100, 5, other) && ring_table_fits(100, 100, 253, other) && ring_table_fits(100, 100, 0, other) &&
                         !ring_table_fits(100, 100, 254, other) && !ring_table_fits(20, 20, 254, 14 * 1024) &&
                         !ring_table_fits(256, 256, 5, 72 * 1024) && !ring_table_fits(180, 180, 5, 16 * 1024) &&
                         ring_table_fits(100, 100, 5, kRingLdsPerBlock - t100) && !ring_table_fits(100, 100, 5, kRingLdsPerBlock - t100 + 1);
    if (!fits_ok || t100 != 10416 || 4 * (other + t100) > 160 * 1024) {
        std::printf("ring_table_fits: a wrong choice (the 100 x 100 table is %u bytes)\n", t100);
        return 1;
    }
    bool covered = off_map >= 1000 && blocked >= 1000 && moves_made >= 1000;
    for (int c = 0; c < kClasses; ++c) covered &= under[c] >= 1000 && target[c] >= 1000;
    if (!covered) {
        std::printf("coverage: %ld off the map, %ld blocked, %ld moves; under %ld %ld %ld %ld, target %ld %ld %ld %ld\n", off_map, blocked,
                    moves_made, under[0], under[1], under[2], under[3], target[0], target[1], target[2], target[3]);
        return 1;
    }
    std::printf("step_ring_check: %ld decode cases (%ld moves off the map, %ld blocked by ground, %ld moves), %ld tables, %ld bias round trips, "
                "9 launch choices, regular == general\n", cases, off_map, blocked, moves_made, tables, trips);
    return 0;
}
