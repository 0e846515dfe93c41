// pow_dot.hpp -- the schedule of k_pow_dot (pow_dot.hip): out = prod_{i<d} base_i^exp_i by ONE ladder whose squarings the d
// bases share (Straus), in a header so that the host build of the CPU tests (tests/hostsim/pow_dot_sim.cpp, COFHE_HOSTSIM)
// compiles the very walk the kernel runs.
//
// Every exponent is read as signed binary digits (the kernel: the non-adjacent form of qf.hpp, times the exponent's sign).
// The walk goes from the top position T = max_i top_i down to 0: one squaring per position below T, then one composition per
// base whose digit at the position is not zero, with the base inverted where the digit is negative.  The first non-zero
// digit met -- at T, by the lowest base that owns one -- is no composition: the accumulator starts as a copy of that base
// (inverted for a negative digit), never as a product with the principal form.  So a walk is T squarings and (non-zero
// digits - 1) multiplications; exponents that are all zero give no operation at all (the kernel then writes the principal form).
#pragma once
#include <stdint.h>

#if defined(COFHE_HOSTSIM)
#define PD_DEV inline
#else
#include <hip/hip_runtime.h>
#define PD_DEV __device__ __forceinline__
#endif

namespace cofhe {

constexpr int POLY_MAX_DEGREE = 8;          // bases of one k_pow_dot record = degree of a polynomial (COFHE_HIP_POLY_MAX_DEGREE)

enum PowDotKind : int { PD_DONE = 0, PD_COPY = 1, PD_SQUARE = 2, PD_MUL = 3 };
struct PowDotOp {
    int kind;       // PD_COPY: acc = base (the start of the walk); PD_SQUARE: acc = acc o acc; PD_MUL: acc = acc o base
    int base;       // PD_COPY, PD_MUL: which base
    int inv;        // PD_COPY, PD_MUL: non-zero = take the base's inverse
};
struct PowDotState {
    int t;          // digit position being served (-1: the walk has ended)
    int i;          // next base to look at on position t
    int started;    // the accumulator holds a value
};

// T = max_i top(i), top(i) the position of base i's highest non-zero digit (-1: exponent zero); -1 when every exponent is zero
template <typename Top>
PD_DEV PowDotState pow_dot_begin(int d, const Top &top) {
    int T = -1;
    for (int i = 0; i < d; i++) {
        const int ti = top(i);
        T = ti > T ? ti : T;
    }
    return PowDotState{T, 0, 0};
}

// the next operation of the walk; digit(i, t) in {-1, 0, 1}.  At most d digit reads per call, and at most
// T + (number of non-zero digits) calls return something other than PD_DONE.
template <typename Digit>
PD_DEV PowDotOp pow_dot_step(PowDotState &s, int d, const Digit &digit) {
    if (s.t < 0) return PowDotOp{PD_DONE, 0, 0};
    while (s.i < d) {
        const int i = s.i++;
        const int dg = digit(i, s.t);
        if (dg != 0) {
            const int kind = s.started ? PD_MUL : PD_COPY;
            s.started = 1;
            return PowDotOp{kind, i, dg < 0 ? 1 : 0};
        }
    }
    // the position is served: the next one opens with a squaring (the accumulator holds a value from position T on)
    s.t--;
    s.i = 0;
    if (s.t < 0) return PowDotOp{PD_DONE, 0, 0};
    return PowDotOp{PD_SQUARE, 0, 0};
}

}  // namespace cofhe
