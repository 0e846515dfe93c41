// spline_table.hpp -- the table builder of the piecewise-polynomial activations (include/cofhe_hip.h states the protocol;
// HIPCryptoSystem::spline_*_tensor and LocalCipherTextMultiplier::evaluate_spline_ciphertext_tensor take its tables).  Host only:
// no GPU, and no GMP beyond what the plaintext type of the caller's choosing needs.
//
// A fixed-point function: x is read as the W = shift + bits bit two's-complement number x / 2^in_frac_bits, the result carries
// out_frac_bits fraction bits.  Piece p (sigma(p) its bits-bit two's-complement reading) has the origin o(p) = sigma(p) 2^shift and
// must serve TWO segments, u = x - o(p) in [0, 2^(shift + 1)): its own and the one above, because the closing step of the protocol
// evaluates an element on its own piece or on the piece below.  make_spline_table interpolates g on that interval at the d + 1
// Chebyshev nodes, in the local coordinate u, and rounds the coefficients to integers at scale 2^out_frac_bits.  Two terms bound
// the error: the interpolation's, max |g^(d+1)| (w / 2)^(d+1) / (2^d (d + 1)!) with w = 2^(shift + 1) / 2^in_frac_bits, and the
// rounding's, sum_i 2^((shift + 1) i) / 2^(out_frac_bits + 1): out_frac_bits has to grow with (shift + 1) d.
//
// The error it reports is the largest |S_p(x) / 2^out_frac_bits - g(x / 2^in_frac_bits)| it saw over the integers the contract
// allows: every x outside the lowest segment (sigma = -2^(bits - 1), where the piece below wraps round to the top piece), on its
// own piece and on the one below -- all of them when a piece's interval has at most 2^16 integers, 2^16 evenly spaced ones and
// the end points otherwise.
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "tensor.hpp"

namespace CoFHE {

struct SplineTable {
    uint32_t bits = 0, shift = 0, degree = 0, in_frac_bits = 0, out_frac_bits = 0;
    std::vector<int64_t> coef;            // [2^bits][degree + 1]: coefficient i of piece p at coef[p (degree + 1) + i]
    double max_error = 0;                 // in units of the function's value
    // S_p(u) / 2^out_frac_bits for the local coordinate u = x - o(p)
    long double value(uint32_t p, long double u) const {
        long double acc = 0;
        for (uint32_t i = degree + 1; i-- > 0;) acc = acc * u + (long double)coef[(size_t)p * (degree + 1) + i];
        return std::ldexp(acc, -(int)out_frac_bits);
    }
    // the table as a plaintext tensor [2^bits, degree + 1] (negative coefficients as negative plaintexts: the engine reduces
    // them mod 2^k); the caller frees the elements, as everywhere in this interface
    template <typename PlainText>
    Tensor<PlainText *> tensor() const {
        Tensor<PlainText *> t({(size_t)1 << bits, (size_t)degree + 1}, nullptr);
        for (size_t m = 0; m < coef.size(); m++) {
            const int64_t c = coef[m];
            t[m] = new PlainText((unsigned long)(c < 0 ? 0 - (uint64_t)c : (uint64_t)c));
            if (c < 0) t[m]->neg();
        }
        return t;
    }
};

template <typename G>
SplineTable make_spline_table(G g, uint32_t bits, uint32_t shift, uint32_t d, uint32_t in_frac_bits, uint32_t out_frac_bits) {
    if (bits == 0 || bits > 12 || d == 0 || d > 8 || (((uint64_t)d + 1) << bits) > 4096)
        throw std::invalid_argument("spline table: 2^bits pieces of degree d, bits >= 1, 1 <= d <= 8, 2^bits (d + 1) <= 4096");
    if (shift + bits > 62 || out_frac_bits > 62) throw std::invalid_argument("spline table: a window and a scale of at most 62 bits");
    SplineTable t;
    t.bits = bits, t.shift = shift, t.degree = d, t.in_frac_bits = in_frac_bits, t.out_frac_bits = out_frac_bits;
    t.coef.assign(((size_t)d + 1) << bits, 0);
    const long double pi = 3.14159265358979323846264338327950288L;
    const long double U = std::ldexp(1.0L, (int)shift + 1);                // the two-segment interval in the local coordinate
    const int64_t half = (int64_t)1 << (bits - 1), seg = (int64_t)1 << shift;
    for (uint32_t p = 0; p < (1u << bits); p++) {
        const int64_t sigma = (int64_t)p >= half ? (int64_t)p - 2 * half : (int64_t)p;
        const long double o = (long double)(sigma * seg);
        // Newton's divided differences at the Chebyshev nodes of v = u / U in [0, 1], then the monomial form in v
        std::vector<long double> v(d + 1), f(d + 1), mono(d + 1, 0.0L);
        for (uint32_t m = 0; m <= d; m++) {
            v[m] = 0.5L * (1.0L + std::cos((2.0L * m + 1.0L) * pi / (2.0L * (d + 1))));
            f[m] = (long double)g((double)std::ldexp(o + v[m] * U, -(int)in_frac_bits));
        }
        for (uint32_t lvl = 1; lvl <= d; lvl++)
            for (uint32_t m = d; m >= lvl; m--) f[m] = (f[m] - f[m - 1]) / (v[m] - v[m - lvl]);
        for (uint32_t m = d + 1; m-- > 0;) {                                // mono = mono (v - v_m) + f_m
            for (uint32_t i = d; i > 0; i--) mono[i] = mono[i - 1] - v[m] * mono[i];
            mono[0] = f[m] - v[m] * mono[0];
        }
        for (uint32_t i = 0; i <= d; i++) {
            const long double c = std::ldexp(mono[i], (int)out_frac_bits - (int)(i * (shift + 1)));
            if (!(std::fabs(c) < 4.0e18L)) throw std::invalid_argument("spline table: a coefficient does not fit 62 bits");
            t.coef[(size_t)p * (d + 1) + i] = (int64_t)std::llround(c);
        }
        // the integers this piece serves: its own segment unless it is the lowest, the one above unless it is the top
        const int64_t lo = sigma == -half ? seg : 0, hi = sigma == half - 1 ? seg : 2 * seg;
        const int64_t step = (hi - lo) > 65536 ? (hi - lo) / 65536 : 1;
        for (int64_t u = lo; u < hi; u = (u + step < hi || u == hi - 1) ? u + step : hi - 1) {
            const long double err = std::fabs(t.value(p, (long double)u) - (long double)g((double)std::ldexp(o + (long double)u, -(int)in_frac_bits)));
            if ((double)err > t.max_error) t.max_error = (double)err;
        }
    }
    return t;
}

}  // namespace CoFHE
