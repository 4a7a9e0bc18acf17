// Host-only check of step_lean.h, the state-only step's action decode and fuel update
// (step_seq.h, step_group_state), against the forms they replaced:
//   lean_fuel(f, scale, moved)  ==  f + (moved ? -scale : -0.0), bit for bit, with scale rounded
//       three times from the FUEL word as the kernel rounds it; FUEL words at every edge and at
//       random, fuel +-0, subnormals, +-inf, +-1e308, the step's own range and random bit patterns
//       that are no NaN; both values of moved;
//   lean_do_move / lean_sel_ok  ==  the error cascade's terms (bad, mv, sel, ok_mv, ok_sel, ok) for
//       every action in [-70, 330] and at the int32 ends, P in {0, 1, 5, 64, 254}, and every
//       combination of nodest, inb and same.
//
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -o step_lean_check tools/step_lean_check.cpp
//   ./step_lean_check   (prints the numbers of cases; exit status 1 on a mismatch)
//
// tests/test_step_lean_host.py builds and runs it (no GPU needed).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../shippingenv_amd/csrc/step_lean.h"

using namespace shipenv;

static const double kFifthPerWord = 0x1.999999999999ap-35;  // env_core.h: fl(0.2) * 2^-32

static uint64_t bits(double d) {
    uint64_t u;
    std::memcpy(&u, &d, sizeof u);
    return u;
}
static double from_bits(uint64_t u) {
    double d;
    std::memcpy(&d, &u, sizeof d);
    return d;
}

// the select form, as step_group_state had it; volatile keeps the three roundings of scale and
// the add apart whatever the compiler would like to fold
static double fuel_select(double f, uint32_t word, bool moved) {
    volatile double fifth = (double)word * kFifthPerWord;
    volatile double noise = -0.1 + fifth;
    volatile double scale = 1.0 + noise;
    volatile double term = moved ? -scale : -0.0;
    return f + term;
}
static double fuel_lean(double f, uint32_t word, bool moved) {
    volatile double fifth = (double)word * kFifthPerWord;
    volatile double noise = -0.1 + fifth;
    volatile double scale = 1.0 + noise;
    return lean_fuel(f, scale, moved);
}

// the error cascade's terms, as step_group_state had them (val wraps as the device's does)
struct Decoded {
    bool do_move, sel_ok;
};
static Decoded decode_cascade(int act, int P, bool nodest, bool inb, bool same) {
    const bool bad = act < -4;
    const bool mv_t = act < 4, mv_f = !mv_t;
    const bool sel_t = (long long)act < 4ll + P;
    const bool ok_mv = mv_t & !nodest & inb;
    const bool ok_sel = mv_f & sel_t & !same;
    const bool ok = !bad & (P != 0) & (ok_mv | ok_sel);
    return Decoded{bool(ok & mv_t), bool(ok & mv_f & sel_t)};
}

int main() {
    uint64_t x = 0x2545f4914f6cdd1dull;  // xorshift64*
    auto next = [&x] {
        x ^= x >> 12;
        x ^= x << 25;
        x ^= x >> 27;
        return x * 0x2545f4914f6cdd1dull;
    };
    // ---- fuel
    std::vector<uint32_t> words = {0u, 1u, 2u, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xfffffffeu, 0xffffffffu};
    for (int b = 0; b < 32; ++b) {
        words.push_back(1u << b);
        words.push_back(~(1u << b));
        words.push_back((1u << b) - 1u);
    }
    std::vector<double> fuels = {0.0, -0.0, 1e308, -1e308, 1.0, -1.0, 0.9, 1.1, 200.0, 0.1, 100.125};
    fuels.push_back(from_bits(0x7ff0000000000000ull));  // +inf
    fuels.push_back(from_bits(0xfff0000000000000ull));  // -inf
    fuels.push_back(from_bits(0x7fefffffffffffffull));  // the largest finite
    for (uint64_t m : {1ull, 2ull, 0x8000000000000ull, 0xfffffffffffffull, 0x10000000000000ull})  // subnormals, the least normal
        for (uint64_t s : {0ull, 1ull << 63}) fuels.push_back(from_bits(s | m));
    long fuel_cases = 0, fuel_moved = 0, fuel_special = 0;
    auto fuel_check = [&](double f, uint32_t wd) {
        for (int moved = 0; moved < 2; ++moved) {
            const double a = fuel_select(f, wd, moved), b = fuel_lean(f, wd, moved);
            ++fuel_cases;
            fuel_moved += moved;
            if (bits(a) != bits(b)) {
                std::printf("fuel differs: f %016llx word %08x moved %d: select %016llx fma %016llx\n",
                            (unsigned long long)bits(f), wd, moved, (unsigned long long)bits(a), (unsigned long long)bits(b));
                return false;
            }
        }
        return true;
    };
    for (double f : fuels)
        for (uint32_t wd : words) {
            ++fuel_special;
            if (!fuel_check(f, wd)) return 1;
        }
    for (double f : fuels)
        for (int i = 0; i < 2000; ++i)
            if (!fuel_check(f, (uint32_t)next())) return 1;
    for (long i = 0; i < 5200000; ++i) {
        double f;
        switch (i & 3) {
        case 0:  // a random bit pattern that is no NaN
            do f = from_bits(next());
            while (f != f);
            break;
        case 1:  // the step's own range, 2^-11 apart and off that grid
            f = (double)(next() % 600000) * 0x1p-11 + ((i & 4) ? (double)(uint32_t)next() * 0x1p-60 : 0.0);
            break;
        case 2:  // around the cost itself: the difference cancels
            f = 0.9 + (double)(uint32_t)next() * kFifthPerWord;
            break;
        default:  // subnormal and tiny
            f = from_bits(next() & 0x801fffffffffffffull);
        }
        const uint32_t wd = (i & 8) ? words[next() % words.size()] : (uint32_t)next();
        if (!fuel_check(f, wd)) return 1;
    }
    // ---- decode
    std::vector<int> acts;
    for (int a = -70; a <= 330; ++a) acts.push_back(a);
    const int32_t lo = INT32_MIN, hi = INT32_MAX;
    for (int d = 0; d < 8; ++d) {
        acts.push_back(lo + d);
        acts.push_back(hi - d);
    }
    for (int d = 250; d < 262; ++d) acts.push_back(hi - d);  // act + 4 + P wraps there for P = 254
    long dec_cases = 0, dec_moves = 0, dec_sels = 0;
    for (int P : {0, 1, 5, 64, 254})
        for (int act : acts)
            for (int c = 0; c < 8; ++c) {
                const bool nodest = c & 1, inb = c & 2, same = c & 4;
                const Decoded want = decode_cascade(act, P, nodest, inb, same);
                const bool mv = lean_do_move(act, P, nodest, inb), sel = lean_sel_ok(act, P, same);
                ++dec_cases;
                dec_moves += mv;
                dec_sels += sel;
                if (mv != want.do_move || sel != want.sel_ok) {
                    std::printf("decode differs: act %d P %d nodest %d inb %d same %d: cascade %d %d, lean %d %d\n", act, P,
                                nodest, inb, same, want.do_move, want.sel_ok, mv, sel);
                    return 1;
                }
            }
    if (fuel_cases < 10000000 || dec_moves < 50 || dec_sels < 500) {
        std::printf("coverage: %ld fuel cases, %ld passed moves, %ld passed selects\n", fuel_cases, dec_moves, dec_sels);
        return 1;
    }
    std::printf("step_lean_check: %ld fuel cases (%ld at word and value edges, %ld movers), %ld decode cases (%ld moves, %ld selects), lean == former\n",
                fuel_cases, 2 * fuel_special, fuel_moved, dec_cases, dec_moves, dec_sels);
    return 0;
}
