// nav_host_check — the navigator's host-only table builder (shippingenv_amd/csrc/navfield.h) as a
// stand-alone program, so that it can run under the host sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o tools/nav_host_check tools/nav_host_check.cpp    (one line)
//   tools/nav_host_check
//
// It builds field and dir for a 1 x 1 map with its one port, a 1 x 12 row, the 256 x 256
// serpentine and a 256 x 256 map with 254 ports (the ABI's limits), into buffers of exactly
// P * H * W entries, and checks the field laws on each: 0 on the port's cell only, neighbouring
// finite cells differ by at most 1, a finite cell other than the port has a neighbour one step
// closer and dir names the first such neighbour, ground is infinite, dir is none exactly where no
// neighbour is finite. It also checks the argument errors. Exit status 0 and "nav_host_check: ok"
// when everything holds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../shippingenv_amd/csrc/navfield.h"

namespace nav = shipenv_nav;

static int g_failed = 0;

#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            if (g_failed++ < 20) {               \
                fprintf(stderr, "FAILED %s: ", #cond); \
                fprintf(stderr, __VA_ARGS__);    \
                fprintf(stderr, "\n");           \
            }                                    \
        }                                        \
    } while (0)

struct World {
    const char* name;
    int32_t H, W;
    std::vector<uint8_t> water;
    std::vector<int32_t> px, py;
};

static void check_world(const World& w, int32_t want_longest) {
    const int32_t P = (int32_t)w.px.size();
    const size_t cells = (size_t)w.H * (size_t)w.W;
    std::vector<uint16_t> field(cells * (size_t)P);
    std::vector<uint8_t> dir(cells * (size_t)P);
    std::string err;
    const int rc = nav::build_tables(w.H, w.W, w.water.data(), P, w.px.data(), w.py.data(), field.data(),
                                     dir.data(), err);
    CHECK(rc == 0, "%s: build_tables: %s", w.name, err.c_str());
    if (rc) return;
    std::vector<uint8_t> open(w.water);
    for (auto& v : open) v = v ? 1 : 0;
    for (int p = 0; p < P; ++p) open[(size_t)w.px[p] * w.W + w.py[p]] = 1;
    int32_t longest = 0;
    for (int p = 0; p < P; ++p) {
        const uint16_t* f = field.data() + (size_t)p * cells;
        const uint8_t* d = dir.data() + (size_t)p * cells;
        for (int32_t x = 0; x < w.H; ++x)
            for (int32_t y = 0; y < w.W; ++y) {
                const size_t c = (size_t)x * w.W + y;
                const bool port = x == w.px[p] && y == w.py[p];
                CHECK((f[c] == 0) == port, "%s: port %d cell (%d, %d) field %u", w.name, p, x, y, f[c]);
                if (!open[c]) CHECK(f[c] == nav::kInf, "%s: ground (%d, %d) is finite", w.name, x, y);
                int best = nav::kInf, pick = nav::kNone;
                for (int k = 0; k < 4; ++k) {
                    const int32_t nx = x + nav::kDx[k], ny = y + nav::kDy[k];
                    if (nx < 0 || nx >= w.H || ny < 0 || ny >= w.W) continue;
                    const uint16_t g = f[(size_t)nx * w.W + ny];
                    if (g < best) {
                        best = g;
                        pick = k;
                    }
                    if (f[c] != nav::kInf && g != nav::kInf)
                        CHECK(abs((int)f[c] - (int)g) <= 1, "%s: port %d (%d, %d) and its neighbour %d differ by more than 1",
                              w.name, p, x, y, k);
                    if (f[c] != nav::kInf && open[(size_t)nx * w.W + ny])
                        CHECK(g != nav::kInf, "%s: port %d (%d, %d): an open neighbour of a finite cell is infinite", w.name, p, x, y);
                }
                CHECK(d[c] == pick, "%s: port %d (%d, %d) dir %u, the rule gives %d", w.name, p, x, y, d[c], pick);
                if (f[c] != nav::kInf && !port) CHECK(best == f[c] - 1, "%s: port %d (%d, %d) has no neighbour one step closer", w.name, p, x, y);
                if (f[c] != nav::kInf && f[c] > longest) longest = f[c];
            }
    }
    CHECK(longest < nav::kInf, "%s: longest %d", w.name, longest);
    if (want_longest >= 0) CHECK(longest == want_longest, "%s: longest %d, expected %d", w.name, longest, want_longest);
    const int32_t leg = nav::max_leg(w.H, w.W, P, w.px.data(), w.py.data(), field.data());
    CHECK(leg <= longest, "%s: max_leg %d past the longest value %d", w.name, leg, longest);
    printf("%-8s %3d x %3d, %3d ports: longest field value %d, max_leg %d\n", w.name, w.H, w.W, P, longest, leg);
}

int main() {
    World dot{"dot", 1, 1, {0}, {0}, {0}};  // the one cell is ground under its port
    check_world(dot, 0);

    World row{"row", 1, 12, std::vector<uint8_t>(12, 1), {0, 0}, {1, 10}};
    check_world(row, 10);

    World snake{"snake", 256, 256, std::vector<uint8_t>(256 * 256, 1), {0, 254}, {0, 0}};
    for (int x = 1; x < 256; x += 2)
        for (int y = 0; y < 256; ++y)
            if (y != (x % 4 == 1 ? 255 : 0)) snake.water[(size_t)x * 256 + y] = 0;
    check_world(snake, 128 * 255 + 127 * 2 + 1);

    World big{"limits", 256, 256, std::vector<uint8_t>(256 * 256), {}, {}};
    uint32_t lcg = 12345u;
    for (auto& v : big.water) {
        lcg = lcg * 1664525u + 1013904223u;
        v = (lcg >> 24) < 154 ? 1 : 0;  // six cells in ten are water: many components
    }
    for (int p = 0; p < 254; ++p) {
        lcg = lcg * 1664525u + 1013904223u;
        big.px.push_back((int32_t)((lcg >> 8) & 255u));
        big.py.push_back((int32_t)((lcg >> 16) & 255u));
    }
    big.px[253] = big.px[0];  // two ports on one cell
    big.py[253] = big.py[0];
    check_world(big, -1);

    // the argument errors, and P = 0
    std::string err;
    std::vector<uint8_t> w4(12, 1);
    const int32_t px[2] = {1, 2}, py[2] = {2, 3}, bad[2] = {1, 3};
    uint16_t f[24];
    uint8_t d[24];
    CHECK(nav::build_tables(3, 4, w4.data(), 0, nullptr, nullptr, nullptr, nullptr, err) == 0, "P = 0");
    CHECK(nav::build_tables(3, 4, w4.data(), 2, px, py, f, nullptr, err) == 0, "no dir");
    CHECK(nav::build_tables(3, 4, w4.data(), 2, px, py, nullptr, d, err) == 0, "no field");
    CHECK(nav::build_tables(0, 4, w4.data(), 2, px, py, f, d, err) == -1, "H = 0");
    CHECK(nav::build_tables(3, 257, w4.data(), 2, px, py, f, d, err) == -1, "W = 257");
    CHECK(nav::build_tables(3, 4, nullptr, 2, px, py, f, d, err) == -1, "null water");
    CHECK(nav::build_tables(3, 4, w4.data(), 255, px, py, f, d, err) == -1, "P = 255");
    CHECK(nav::build_tables(3, 4, w4.data(), -1, px, py, f, d, err) == -1, "P = -1");
    CHECK(nav::build_tables(3, 4, w4.data(), 2, nullptr, py, f, d, err) == -1, "null port_x");
    CHECK(nav::build_tables(3, 4, w4.data(), 2, bad, py, f, d, err) == -1, "a port outside the map");

    if (g_failed) {
        fprintf(stderr, "nav_host_check: %d checks failed\n", g_failed);
        return 1;
    }
    printf("nav_host_check: ok\n");
    return 0;
}
