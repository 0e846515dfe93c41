// Host build of k_pow_dot's schedule (cofhe_amd/csrc/pow_dot.hpp) with COFHE_HOSTSIM: the very walk the kernel runs, written
// out as a list of operations for signed digits the caller supplies.  TEST INFRASTRUCTURE ONLY; not linked into the product
// library.
#define COFHE_HOSTSIM 1
#include "../../cofhe_amd/csrc/pow_dot.hpp"

using namespace cofhe;

extern "C" {
int pow_dot_sim_max_degree(void) { return POLY_MAX_DEGREE; }
// digits: d rows of npos signed digits (row i: the digits of exponent i, position 0 first, sign of the exponent applied).
// ops[3 r .. 3 r + 2] = kind (1 copy, 2 square, 3 multiply), base, inverted, for the walk's operations in order; returns their
// number, or -1 when more than cap would be written
int pow_dot_sim_walk(const int8_t *digits, int d, int npos, int32_t *ops, int cap) {
    auto digit = [&](int i, int t) { return (int)digits[(long)i * npos + t]; };
    PowDotState s = pow_dot_begin(d, [&](int i) {
        int top = -1;
        for (int t = 0; t < npos; t++)
            if (digit(i, t) != 0) top = t;
        return top;
    });
    int n = 0;
    while (true) {
        const PowDotOp op = pow_dot_step(s, d, digit);
        if (op.kind == PD_DONE) return n;
        if (n >= cap) return -1;
        ops[3 * n + 0] = op.kind;
        ops[3 * n + 1] = op.base;
        ops[3 * n + 2] = op.inv;
        n++;
    }
}
}
