#pragma once
// qnet_image.h — the layouts of the packed network images: QnetDims (the bf16 image, full and
// compact fc3 rows), QnetX3Dims (the split-bf16 image), and the maps both packers and the kernels
// share: fc1's column of a fragment element (fc1_col), the accumulator row of a k-step element
// (acc_row) and the split-bf16 fc1 slots (Fc1Slot, x3_fc1_slot).
//
// A fragment of shipenv.hip's translation unit, included inside qpolicy.h's anonymous
// namespace, first of its fragments: not a stand-alone header. Uses nothing but <stdint.h>.

constexpr int kQHidden = 128;     // DQNNetwork hidden_size (dqn.py:24, default 128)

// Packed network image (bytes). Fragments are 64 lanes x 8 bf16 = 1 KB.
// Two layouts of fc3's rows:
// * full: row r is action r (A = 4 + P + 250 rows), for the Q output (q_out);
// * compact: only the actions some env can ever take, in ascending order: the moves and
//   SELECT rows [0, 4 + P), then TAKE_CARGO amounts 1..cmax and TAKE_FUEL amounts
//   1..fmax, cmax / fmax the largest stocks of the world's ports (add_port draws 5..20,
//   so 49 rows and 2 tiles at P = 5 instead of 3 of the 9 full tiles with a valid row).
//   The first maximum in compact rows is the first in actions (the map is increasing).
struct QnetDims {
    int32_t P, A, rows, mt3;  // ports, actions, fc3 rows of this layout, its row tiles
    int32_t compact, cmax;    // the layout; TAKE_CARGO rows in the compact one
    __host__ __device__ int in1() const { return 6 + 4 * P; }
    // action of fc3 row r (utils/preprocessing.py:111-137)
    __host__ __device__ int action_of_row(int r) const {
        if (!compact || r < 4 + P) return r;
        return r < 4 + P + cmax ? r + 1 : r + 51 - cmax;
    }
    // row of TAKE_CARGO amount 1 and of TAKE_FUEL amount 1
    __host__ __device__ int cargo_row1() const { return compact ? 4 + P : 5 + P; }
    __host__ __device__ int fuel_row1() const { return compact ? 4 + P + cmax : 55 + P; }
    __host__ __device__ int w1() const { return 0; }                    // 4 fc1 tiles
    __host__ __device__ int w2() const { return 4 * 1024; }              // 4 x 4 x 2 fc2 fragments
    __host__ __device__ int w3() const { return w2() + 32 * 1024; }      // mt3 x 4 x 2 fc3 fragments
    __host__ __device__ int b1() const { return w3() + mt3 * 8 * 1024; } // 128 f32, port block folded
    __host__ __device__ int b2() const { return b1() + 4 * kQHidden; }
    __host__ __device__ int b3() const { return b2() + 4 * kQHidden; }   // mt3 * 32 f32 (0 beyond A)
    __host__ __device__ int same() const { return b3() + mt3 * 128; }    // P uint64: ports on port p's cell
    __host__ __device__ int regm() const { return same() + 8 * P; }      // mt3 uint32: fc3 epilogue regs
    __host__ __device__ int bytes() const { return (regm() + 4 * mt3 + 15) & ~15; }
};

QnetDims qnet_dims(int P, bool compact = false, int cmax = 0, int fmax = 0) {
    QnetDims q;
    q.P = P;
    q.A = 4 + P + 250;  // utils/preprocessing.py:93-108
    q.compact = compact ? 1 : 0;
    q.cmax = compact ? cmax : 49;
    q.rows = compact ? 4 + P + cmax + fmax : q.A;
    q.mt3 = (q.rows + 31) / 32;
    return q;
}

// fc1 input column of fragment element j: x, y, fuel (hi), fuel (lo), "cargo" = fuel
// (hi, lo; environment.py:206), origin, dest (utils/preprocessing.py:51-58)
__device__ __forceinline__ int fc1_col(int j) {
    return j < 2 ? j : (j < 4 ? 2 : (j < 6 ? 3 : j - 2));
}

__device__ __forceinline__ int acc_row(int s, int j, int h) { return 16 * s + 8 * (j >> 2) + 4 * h + (j & 3); }

struct QnetX3Dims {
    QnetDims q;
    int32_t zrow;  // bf16x8 index, at k-step 0 and part 0, of a zero row of fc3's last tile (lane 31 of it), or -1
    __host__ __device__ int w1() const { return 0; }  // fc1: bf16 fragments [mt][2 steps][lane] (8 KB)
    __host__ __device__ int w2() const { return 8192; }                 // [mt][kt][s][part] bf16 fragments: 96 KB
    __host__ __device__ int b1() const { return w2() + 96 * 1024; }
    __host__ __device__ int b2() const { return b1() + 4 * kQHidden; }
    __host__ __device__ int b3() const { return b2() + 4 * kQHidden; }  // mt3 * 32 f32
    __host__ __device__ int same() const { return b3() + q.mt3 * 128; }
    __host__ __device__ int regm() const { return same() + 8 * q.P; }
    __host__ __device__ int w3() const { return (regm() + 4 * q.mt3 + 15) & ~15; }  // mt3 x 24 KB, last
    __host__ __device__ int bytes() const { return w3() + q.mt3 * 24 * 1024; }
};

// fc1 on bf16 MFMA: the six dynamic columns' products as 24 of the 32 k
// slots of two v_mfma_f32_32x32x16_bf16 per row tile. Slot k (step k >> 4, lane half
// (k >> 3) & 1, element k & 7) holds weight part wp of column col times input part xp:
// x, y, origin, dest are exact in bf16 (|v| <= 255), so they take w0 x + w1 x + w2 x; the
// fuel column (2) and the "cargo" = fuel column (3, environment.py:206) take the six split
// products of w and the fuel f32. Columns: 0 x, 1 y, 2 fuel, 3 cargo, 4 origin, 5 dest.
struct Fc1Slot {
    int8_t col, wp, xp;  // xp: -1 = the exact input, else the fuel part
};
// Slots 24-31 are zero. (fc1's bias folded into slots 24-26 against inputs of 1.0 measured even
// or slower, profiles/r05/ab_policy_f32_bias_fold.jsonl; the bf16 kernel's 64-bit valid-row
// masks here 0.2724 vs 0.2630 ms per call, profiles/r05/ab_policy_f32_valid64.jsonl.)

__host__ __device__ constexpr Fc1Slot x3_fc1_slot(int k) {
    constexpr Fc1Slot t[24] = {{0, 0, -1}, {1, 0, -1}, {4, 0, -1}, {5, 0, -1}, {0, 1, -1}, {1, 1, -1}, {4, 1, -1}, {5, 1, -1},
                               {0, 2, -1}, {1, 2, -1}, {4, 2, -1}, {5, 2, -1}, {2, 0, 0},  {2, 0, 1},  {2, 1, 0},  {2, 0, 2},
                               {2, 1, 1},  {2, 2, 0},  {3, 0, 0},  {3, 0, 1},  {3, 1, 0},  {3, 0, 2},  {3, 1, 1},  {3, 2, 0}};
    return k < 24 ? t[k] : Fc1Slot{-1, 0, 0};
}
