#pragma once
// navfield.h — the navigator's route tables, built on the host: for every port the number of
// moves over non-ground cells from every cell to that port (field), and for every cell the move
// that goes down that field (dir). Host-only C++: no HIP, no device, nothing of shipenv.hip's.
// shipenv.hip includes it for se_nav_build_host and the se_nav handle (nav.h), and
// tools/nav_host_check.cpp includes it alone to run the builder under the host sanitizers.
//
// Cells are c = x * W + y with x the map row, as the world image has them; a port's cell is
// never ground (Entity.PORT is stamped over the map, environment.py:65). The moves are the agent
// index's, k = 0..3 = N (0,-1), E (-1,0), S (0,1), W (1,0) applied to (x, y)
// (utils/preprocessing.py:126).
#include <stdint.h>

#include <string>
#include <vector>

namespace shipenv_nav {

constexpr uint16_t kInf = 0xFFFF;  // SE_NAV_INF: ground, or no path to the port
constexpr uint8_t kNone = 255;     // SE_NAV_NONE: no neighbour with a finite field value
constexpr int kMaxSide = 256;      // SE_MAX_SIDE
constexpr int kMaxPorts = 254;     // SE_MAX_PORTS
constexpr int kDx[4] = {0, -1, 0, 1}, kDy[4] = {-1, 0, 1, 0};

// field[p * H * W + c] and dir[p * H * W + c] for p < P (either may be null: not wanted).
// Returns 0, or -1 (SE_EINVAL) with the reason in err; the checks are se_create's.
//   field  the least number of moves from c to port p's cell over in-map non-ground cells; 0 on
//          the port's cell, kInf on ground and where there is no such path.
//   dir    the k of the in-map neighbour with the smallest finite field value, the lowest k on a
//          tie (a scan in k order with a strict less-than); kNone when no neighbour is finite.
//          On the port's own cell that is a neighbour with field 1: step off and come back (the
//          step tests for an arrival only inside a move). A ground cell on a coast gets the move
//          onto the field; no ship stands there unless it was placed by hand, and that move is
//          legal.
// A finite value cannot reach kInf for H, W <= 256: a shortest path is an induced path of the
// grid graph (two of its cells that are neighbours are consecutive on it, or there were a
// shorter one), so it holds at most three cells of any 2 x 2 block, and below 256 x 256 cells
// H * W - 1 < kInf anyway; at 256 x 256 the 128 x 128 disjoint blocks allow 49152 cells, a
// value of 49151 at most. The values are computed in int32 and checked all the same.
inline int build_tables(int32_t H, int32_t W, const uint8_t* water, int32_t P, const int32_t* port_x,
                        const int32_t* port_y, uint16_t* field, uint8_t* dir, std::string& err) {
    if (H < 1 || W < 1 || H > kMaxSide || W > kMaxSide) {
        err = "map sides must be in [1, 256]";
        return -1;
    }
    if (!water) {
        err = "null water map";
        return -1;
    }
    if (P < 0 || P > kMaxPorts) {
        err = "P must be in [0, 254]";
        return -1;
    }
    if (P > 0 && (!port_x || !port_y)) {
        err = "null port arrays";
        return -1;
    }
    for (int p = 0; p < P; ++p)
        if (port_x[p] < 0 || port_x[p] >= H || port_y[p] < 0 || port_y[p] >= W) {
            err = "Coordinates not within map";
            return -1;
        }
    const int32_t cells = H * W;
    std::vector<uint8_t> open((size_t)cells);  // 1: a ship may stand here
    for (int32_t c = 0; c < cells; ++c) open[(size_t)c] = water[c] ? 1 : 0;
    for (int p = 0; p < P; ++p) open[(size_t)port_x[p] * W + port_y[p]] = 1;
    std::vector<int32_t> dist((size_t)cells), queue((size_t)cells);
    for (int p = 0; p < P; ++p) {
        dist.assign((size_t)cells, -1);
        int32_t head = 0, tail = 0;
        const int32_t start = port_x[p] * W + port_y[p];
        dist[(size_t)start] = 0;
        queue[(size_t)tail++] = start;
        while (head < tail) {  // breadth first: every cell enters the queue once
            const int32_t c = queue[(size_t)head++];
            const int32_t x = c / W, y = c % W;
            for (int k = 0; k < 4; ++k) {
                const int32_t nx = x + kDx[k], ny = y + kDy[k];
                if (nx < 0 || nx >= H || ny < 0 || ny >= W) continue;
                const int32_t nc = nx * W + ny;
                if (!open[(size_t)nc] || dist[(size_t)nc] >= 0) continue;
                dist[(size_t)nc] = dist[(size_t)c] + 1;
                if (dist[(size_t)nc] >= (int32_t)kInf) {
                    err = "a route field value does not fit 16 bits";
                    return -1;
                }
                queue[(size_t)tail++] = nc;
            }
        }
        const size_t base = (size_t)p * (size_t)cells;
        if (field)
            for (int32_t c = 0; c < cells; ++c)
                field[base + (size_t)c] = dist[(size_t)c] < 0 ? kInf : (uint16_t)dist[(size_t)c];
        if (dir)
            for (int32_t c = 0; c < cells; ++c) {
                const int32_t x = c / W, y = c % W;
                int32_t best = (int32_t)kInf;
                uint8_t pick = kNone;
                for (int k = 0; k < 4; ++k) {
                    const int32_t nx = x + kDx[k], ny = y + kDy[k];
                    if (nx < 0 || nx >= H || ny < 0 || ny >= W) continue;
                    const int32_t d = dist[(size_t)nx * W + ny];
                    if (d >= 0 && d < best) {
                        best = d;
                        pick = (uint8_t)k;
                    }
                }
                dir[base + (size_t)c] = pick;
            }
    }
    return 0;
}

// The largest finite field value between two ports' cells, 0 if there is none.
inline int32_t max_leg(int32_t H, int32_t W, int32_t P, const int32_t* port_x, const int32_t* port_y,
                       const uint16_t* field) {
    int32_t best = 0;
    const size_t cells = (size_t)H * (size_t)W;
    for (int p = 0; p < P; ++p)
        for (int q = 0; q < P; ++q) {
            const uint16_t f = field[(size_t)p * cells + (size_t)port_x[q] * W + port_y[q]];
            if (f != kInf && (int32_t)f > best) best = f;
        }
    return best;
}

}  // namespace shipenv_nav
