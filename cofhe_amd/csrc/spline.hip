// spline.hip -- the three kernels of a piecewise-polynomial activation on ciphertext tensors from one opened value (launched by
// abi.hip, declared in kernels.hpp; the protocol, the index arithmetic and the bodies of the two plaintext kernels: spline.hpp).
// k_spline_rows writes the plaintext rows of the spline tuples, the Taylor shifts of the pieces rotated by each element's mask;
// k_spline_powers the powers e, e^2, .., e^d mod 2^k of the opened values; k_spline_close closes the evaluation with the walk of
// k_pow_dot (pow_dot_walk.hpp) over the row of the tuple that the opened value names, and one composition with its constant term.
#include <hip/hip_runtime.h>

#include "pow_dot_walk.hpp"
#include "spline.hpp"

using namespace cofhe;

#ifndef COFHE_WPS
#define COFHE_WPS 4      // minimum waves per SIMD the register allocator must leave room for (as cofhe_hip.hip)
#endif

namespace cofhe_k {

// out[(i 2^bits + j) (d + 1) + c] = coefficient c of the Taylor shift of piece (j + rho_i) mod 2^bits of table i mod n_tab at
// (r_i - o(piece)) mod 2^kbits, rho_i = bits shift .. shift + bits - 1 of r_i: one thread per (element, row), i < n, j < 2^bits,
// c <= d; pieces: n_tab 2^bits (d + 1) exponent records; out must not overlap pieces or r
__global__ void __launch_bounds__(SPL_THREADS) k_spline_rows(const uint32_t *__restrict__ pieces, uint64_t n_tab, const uint32_t *__restrict__ r,
                                                             uint32_t *__restrict__ out, uint64_t n, uint32_t bits, uint32_t shift, uint32_t d,
                                                             uint32_t kbits) {
    const uint64_t idx = (uint64_t)blockIdx.x * SPL_THREADS + threadIdx.x;
    if (idx >= (n << bits)) return;
    spline_rows_element(pieces, n_tab, r, out, idx, bits, shift, (int)d, kbits);
}

// out[(c - 1) n + i] = e[i]^c mod 2^kbits, c = 1 .. d, on exponent records: one thread per element; out must not overlap e
__global__ void __launch_bounds__(SPL_THREADS) k_spline_powers(const uint32_t *__restrict__ e, uint32_t *__restrict__ out, uint64_t n, uint32_t d,
                                                               uint32_t kbits) {
    const uint64_t i = (uint64_t)blockIdx.x * SPL_THREADS + threadIdx.x;
    if (i >= n) return;
    spline_powers_element(e, out, n, i, (int)d, kbits);
}

// out[2 i + h] = q_0 o prod_{c = 1 .. d} q_c^powers[(c - 1) n + i], q_c = tuples[(((i 2^bits + j) (d + 1) + c) 2 + h], j = bits
// shift .. shift + bits - 1 of e[i] mod 2^kbits, i < n, h in {0, 1}: one limb group per output record.  A sequence kernel like
// k_pow_dot, whose walk (pow_dot_walk.hpp) it runs with two changes.  The bases are read in place from row j of the element's
// tuple.  And the constant term [q_0] joins the walk as one more base, the LAST one, whose only digit is a 1 at position 0: the
// last position serves it after the d others, so it is the last composition of the record and one more lockstep round of the
// workgroup, through the walk's one qf_compose.  A record whose powers are all zero (e = 0 mod 2^kbits) has no other digit: its
// walk is the copy that starts it, [q_0] itself.  The running product lives in the OUTPUT record (which therefore must not
// overlap an input: the launcher refuses that); a group without work squares q_1 and stores nothing.
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_spline_close(const uint32_t *__restrict__ e, const uint32_t *__restrict__ powers,
                                                                      const uint32_t *__restrict__ tuples, uint32_t *__restrict__ out, uint64_t n,
                                                                      uint32_t bits, uint32_t shift, uint32_t d, uint32_t kbits,
                                                                      const uint32_t *__restrict__ absdelta, int half_dbits,
                                                                      uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[WG_CTX_LDS_WORDS];
    Ctx c = make_served_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t n_records = 2 * n;
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const bool alive = g0 < n_records;
    const uint64_t g = alive ? g0 : n_records - 1;
    const uint64_t i = g >> 1;
    const int nd = (int)d;
    // coefficient 0 of the selected row, half h of its ciphertext; coefficient c is one ciphertext further each
    const uint64_t row = (i << bits) + spline_index(e + i * EXP_REC_WORDS, shift, bits, kbits);
    const uint32_t *q0 = tuples + (row * (d + 1) * 2 + (g & 1)) * REC_WORDS;
    uint32_t *accp = out + g * REC_WORDS;
    PowDotDigits dig;
    dig.exps = powers + i * EXP_REC_WORDS;
    dig.stride = n * EXP_REC_WORDS;
    PowDotState s = pow_dot_prepare(dig, nd);
    if (s.t < 0) s.t = 0;                                     // the constant term's digit
    pow_dot_walk(
        c, dd, alive, nd + 1, [&](int b, int t) { return b < nd ? dig(b, t) : (t == 0 ? 1 : 0); }, s, accp,
        [&](int b) { return b < nd ? q0 + (uint64_t)(b + 1) * 2 * REC_WORDS : q0; });
}

}  // namespace cofhe_k
