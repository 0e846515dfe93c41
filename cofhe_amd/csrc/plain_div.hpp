// plain_div.hpp -- the body of k_plain_divfloor (divide.hip): the signed floor division of residues mod 2^k by public divisors on
// exponent records,
//   q[e] = floor(s(v[e]) / D[e mod n_div]) mod 2^k,   s(v) the centred residue of v in [-2^(k-1), 2^(k-1)),   1 <= D < 2^(k-1),
// in a header so that the host build of the CPU tests (tests/hostsim/plain_div_sim.cpp, COFHE_HOSTSIM) compiles the very code
// the kernel runs.  It is the one new piece of device arithmetic of a division of ciphertexts by public divisors from one opened
// value (cofhe_hip_div_close_records): both halves of a division pair and the opened value go through it.
//
// One 8-lane limb group per element (lane.hpp), the value in one plane of 1280 bits, the division by mp_divrem<1,1> (mp.hpp):
// k <= 639 leaves more than the headroom that division asks for.  A value enters as its residue in [0, 2^k) exactly as in the
// plaintext matrix product (plain_mm.hpp: pmm_reduce): the low k bits of the magnitude, and 2^k minus that where the sign word
// is set -- so magnitudes of 2^k and above and -0 are fine.  The residue v is negative when bit k - 1 is set; then with
// m = 2^k - v > 0
//   floor(-m / D) = -(floor((m - 1) / D) + 1),   m - 1 = (2^k - 1) - v = ~v,   2^k - (q' + 1) = (2^k - 1) - q' = ~q'
// (complements within k bits): the negative branch is two masked complements around the same unsigned division, no carries.
// The only carry chain is the 2^k - m of a record with a set sign word.  Loads and stores go straight between the record and
// the lanes' registers (lane gl owns words 5 gl .. 5 gl + 4): no LDS beyond what mp_divrem stages.
//
// A divisor is invalid when its record has a set sign word, when its residue is 0 or when it is 2^(k-1) or more: the element's
// quotient is then 0 and CF_ST_DIV_CAP is set in the status word; nothing loops.  The output lies in [0, 2^k) with sign word 0,
// and every word of the record is written.
#pragma once
#include "mp.hpp"
#include "plain_mm.hpp"

namespace cofhe {

constexpr int PDV_GROUPS = WG_GROUPS;           // elements of a k_plain_divfloor workgroup: one limb group each
constexpr int PDV_THREADS = PDV_GROUPS * G;
constexpr uint32_t PDV_MAX_KBITS = 32u * PMM_MAX_LIMBS - 1;      // 639: the bound of the decryption table (2 k + 1 <= 1280)
static_assert(PMM_REC_WORDS <= PLIMBS && PDV_MAX_KBITS < (uint32_t)PLIMBS * 32 - 100, "a record fits one plane with mp_divrem's headroom");

// the low k bits of a record's magnitude, lane gl holding words 5 gl .. 5 gl + 4
CF_DEV Mp<1> pdv_load_magnitude(const Ctx &c, const uint32_t *rec, uint32_t kbits) {
    const int L = pmm_limbs(kbits);
    const uint32_t top = pmm_top_mask(kbits);
    Mp<1> x;
    CF_UNROLL for (int j = 0; j < CH; j++) {
        const int i = c.gl * CH + j;
        const uint32_t w = i < L ? rec[i < L ? i : 0] : 0u;        // L <= 20 < PMM_MAG_WORDS: never the sign word
        x.v[0][j] = i == L - 1 ? w & top : w;
    }
    return x;
}

// (2^k - 1) - x for x < 2^k: the complement within k bits
CF_DEV Mp<1> pdv_complement(const Ctx &c, const Mp<1> &x, uint32_t kbits) {
    const int L = pmm_limbs(kbits);
    const uint32_t top = pmm_top_mask(kbits);
    Mp<1> y;
    CF_UNROLL for (int j = 0; j < CH; j++) {
        const int i = c.gl * CH + j;
        y.v[0][j] = i < L - 1 ? ~x.v[0][j] : (i == L - 1 ? ~x.v[0][j] & top : 0u);
    }
    return y;
}

// the residue in [0, 2^k) of a record: sign word honoured
CF_DEV Mp<1> pdv_load_residue(Ctx &c, const uint32_t *rec, uint32_t kbits) {
    Mp<1> x = pdv_load_magnitude(c, rec, kbits);
    if (rec[PMM_MAG_WORDS] != 0) {                                  // group-uniform: every lane reads the same word
        // 2^k - x = ((2^k - 1) - x) + 1, and 2^k itself (x = 0) reduces to 0
        Mp<1> one;
        mp_set_word(c, one, 1u);
        const Mp<1> nx = pdv_complement(c, x, kbits);
        (void)mp_add(c, x, nx, one);
        const int L = pmm_limbs(kbits);
        const uint32_t top = pmm_top_mask(kbits);
        CF_UNROLL for (int j = 0; j < CH; j++) {
            const int i = c.gl * CH + j;
            x.v[0][j] = i < L - 1 ? x.v[0][j] : (i == L - 1 ? x.v[0][j] & top : 0u);
        }
    }
    return x;
}

// x < 2^k as an exponent record: every word written, sign word 0
CF_DEV void pdv_store(const Ctx &c, const Mp<1> &x, uint32_t *rec) {
    CF_UNROLL for (int j = 0; j < CH; j++) {
        const int i = c.gl * CH + j;
        if (i < PMM_MAG_WORDS) rec[i] = x.v[0][j];
        else if (i == PMM_MAG_WORDS) rec[i] = 0u;
    }
}

// qrec = floor(s(vrec) / drec) mod 2^kbits, 1 <= kbits <= PDV_MAX_KBITS (the launcher's check); every lane of the group calls
// this with the same arguments
CF_DEV void plain_divfloor_element(Ctx &c, const uint32_t *vrec, const uint32_t *drec, uint32_t *qrec, uint32_t kbits) {
    Mp<1> q;
    const Mp<1> den = pdv_load_magnitude(c, drec, kbits);
    const int sign_limb = (int)((kbits - 1) >> 5);
    const uint32_t sign_bit = 1u << ((kbits - 1) & 31);
    const bool bad = drec[PMM_MAG_WORDS] != 0 || mp_is_zero(c, den) || (mp_get_limb(c, den, sign_limb) & sign_bit) != 0;
    if (bad) {
        CF_STATUS(c, CF_ST_DIV_CAP);
        mp_zero(q);
        pdv_store(c, q, qrec);
        return;
    }
    Mp<1> num = pdv_load_residue(c, vrec, kbits);
    const bool neg = (mp_get_limb(c, num, sign_limb) & sign_bit) != 0;
    if (neg) num = pdv_complement(c, num, kbits);                   // m - 1 of the magnitude m = 2^k - v
    mp_divrem<1, 1>(c, num, den, q);
    if (neg) q = pdv_complement(c, q, kbits);                       // 2^k - (q' + 1)
    pdv_store(c, q, qrec);
}

}  // namespace cofhe
