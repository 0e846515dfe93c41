// kernels.hpp -- one declaration of every kernel that abi.hip launches.  The definitions, with their
// __launch_bounds__, are in cofhe_hip.hip (the throughput kernels, in three COFHE_PART passes) and wide.hip
// (the latency kernels); wire.hip launches its own kernels.  A declaration that matches no definition is an
// undefined symbol when the library is loaded (tests/test_cabi.py).  comb.hip holds the two kernels of the fixed-base comb,
// affine.hip the ciphertext difference and the record inverse, matmul_left.hip the record transpose and the plaintext
// matrix product, conv.hip the convolution's level 0, its patch gather and its filter expansion, conv_ct.hip the plaintext
// convolution and the patch gather of a plaintext image for ciphertext filters, pow_dot.hip the multi-exponentiation
// and the Taylor shift of the polynomial evaluation, divide.hip the signed floor division on exponent records, divide_exact.hip
// the quotient with its remainder, the rows and the entry selection of the exact division by small divisors, lut.hip the row
// rotation and the entry selection of the table lookups, spline.hip the rows, the powers and the closing walk of the
// piecewise-polynomial activations, view.hip the affine view and the index gather that rearrange resident tensors, compare.hip the
// rows and the closing compositions of the digit comparisons.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "comb.hpp"
#include "conv.hpp"
#include "view.hpp"

namespace cofhe_k {

// tensor addition and form validation (cofhe_hip.hip)
__global__ void k_compose_wg(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out, uint64_t n,
                             const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);
__global__ void k_compose_wg3(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out, uint64_t n,
                              const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);
__global__ void k_validate_forms(const uint32_t *__restrict__ recs, uint64_t n, const uint32_t *__restrict__ absdelta, uint32_t *__restrict__ err);
__global__ void k_c1_distinct(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint64_t n_ct, uint32_t *__restrict__ flag);
__global__ void k_c1_spread(uint32_t *__restrict__ out, uint64_t n_ct, const uint32_t *__restrict__ flag);
__global__ void k_spread_records(uint32_t *__restrict__ recs, uint64_t n);
__global__ void k_add_ct(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out, uint64_t n_ct,
                         const uint32_t *__restrict__ flag, const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status,
                         uint32_t only);
__global__ void k_add_ct3(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out, uint64_t n_ct,
                          const uint32_t *__restrict__ flag, const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status,
                          uint32_t only);

// powering, encryption and the pairwise product trees (cofhe_hip.hip)
__global__ void k_pow(const uint32_t *__restrict__ base, const uint32_t *__restrict__ exps, uint32_t *__restrict__ out, uint64_t n_records,
                      uint32_t base_stride, uint32_t exp_mode, const uint32_t *__restrict__ one_rec, const uint32_t *__restrict__ absdelta,
                      int half_dbits, uint32_t *__restrict__ status);
__global__ void k_square_chain(const uint32_t *__restrict__ base, uint32_t *__restrict__ table, uint32_t len, const uint32_t *__restrict__ absdelta,
                               int half_dbits, uint32_t *__restrict__ status);
__global__ void k_gather_signed(const uint64_t *__restrict__ tabs, const uint32_t *__restrict__ idx, uint64_t n, const uint32_t *__restrict__ one_rec,
                                uint32_t *__restrict__ out);
__global__ void k_encrypt_select(const uint32_t *__restrict__ plain, uint64_t n_ct, int kbits, uint32_t cap, uint32_t *__restrict__ idx,
                                 uint32_t *__restrict__ max_slots);
__global__ void k_zip_ciphertexts(const uint32_t *__restrict__ c1, const uint32_t *__restrict__ c2, uint64_t n_ct, uint32_t *__restrict__ out);
__global__ void k_compose_pairs(const uint32_t *__restrict__ x, const uint32_t *__restrict__ pad, uint32_t *__restrict__ out, uint32_t n, uint32_t m,
                                uint32_t q, uint32_t pad_by_h, const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);
__global__ void k_accumulate(const uint32_t *__restrict__ x, const uint32_t *__restrict__ zero, uint32_t *__restrict__ out, uint32_t n, uint32_t m,
                             uint32_t p, const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);

// the plaintext-matrix x ciphertext-matrix product: chains and product tree (cofhe_hip.hip)
__global__ void k_exp_maxbits(const uint32_t *__restrict__ exps, uint64_t n_exps, uint32_t *__restrict__ maxbits);
__global__ void k_wnaf_digits(const uint32_t *__restrict__ exps, uint64_t n_exps, uint32_t w, int8_t *__restrict__ digits,
                              uint32_t *__restrict__ maxlen);
__global__ void k_pow_table(const uint32_t *__restrict__ base, uint32_t *__restrict__ table, uint64_t n_records, uint32_t tw,
                            const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);
__global__ void k_pow_table3(const uint32_t *__restrict__ base, uint32_t *__restrict__ table, uint64_t n_records, uint32_t tw,
                             const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);
__global__ void k_matmul_schedule(const int8_t *__restrict__ digits, const uint32_t *__restrict__ maxlen, uint32_t m, uint32_t p, uint32_t segs,
                                  uint32_t rcap, uint32_t *__restrict__ ops, uint32_t *__restrict__ counts, uint32_t *__restrict__ status);
__global__ void k_scal_matmul_wnaf(const uint32_t *__restrict__ table, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ counts,
                                   uint32_t rcap, const uint32_t *__restrict__ zero, uint32_t *__restrict__ out, uint32_t n, uint32_t m, uint32_t p,
                                   uint32_t tw, uint32_t segs, const uint32_t *__restrict__ one_rec, const uint32_t *__restrict__ absdelta,
                                   int half_dbits, uint32_t *__restrict__ status);
__global__ void k_scal_matmul_wnaf3(const uint32_t *__restrict__ table, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ counts,
                                    uint32_t rcap, const uint32_t *__restrict__ zero, uint32_t *__restrict__ out, uint32_t n, uint32_t m, uint32_t p,
                                    uint32_t tw, uint32_t segs, const uint32_t *__restrict__ one_rec, const uint32_t *__restrict__ absdelta,
                                    int half_dbits, uint32_t *__restrict__ status);
__global__ void k_tree_count(const int8_t *__restrict__ digits, const uint32_t *__restrict__ maxlen, uint32_t m, uint32_t p,
                             uint32_t *__restrict__ cnt);
__global__ void k_tree_plan(const uint32_t *__restrict__ maxlen, uint32_t p, uint32_t S_cap, uint32_t *__restrict__ c, uint32_t *__restrict__ off,
                            uint32_t *__restrict__ info);
__global__ void k_tree_fill(const int8_t *__restrict__ digits, uint32_t m, uint32_t p, uint32_t S_cap, const uint32_t *__restrict__ c,
                            const uint32_t *__restrict__ off, const uint32_t *__restrict__ info, uint32_t *__restrict__ ent0,
                            uint32_t *__restrict__ maps);
__global__ void k_tree_horner_schedule(const uint32_t *__restrict__ maxlen, uint32_t p, uint32_t S_cap, const uint32_t *__restrict__ c,
                                       const uint32_t *__restrict__ off, const uint32_t *__restrict__ info, uint32_t rcap, uint32_t *__restrict__ ops,
                                       uint32_t *__restrict__ counts, uint32_t *__restrict__ status);
__global__ void k_tree_level(const uint32_t *__restrict__ src, uint32_t from_table, const uint32_t *__restrict__ ent0,
                             const uint32_t *__restrict__ off_cur, const uint32_t *__restrict__ off_next, const uint32_t *__restrict__ map_next,
                             uint32_t n_cur, uint32_t n_next, uint32_t rows, uint32_t m, uint32_t tw, uint32_t *__restrict__ dst,
                             const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);

// shared-base ladders and decryption (cofhe_hip.hip)
__global__ void k_pow_shared(const uint32_t *__restrict__ base, const int8_t *__restrict__ digits, const uint32_t *__restrict__ maxlen,
                             uint32_t *__restrict__ table, uint32_t *__restrict__ out, uint64_t n_items, uint32_t base_stride, uint32_t tw,
                             const uint32_t *__restrict__ one_rec, const uint32_t *__restrict__ absdelta, int half_dbits,
                             uint32_t *__restrict__ status);
__global__ void k_pow_shared_solo(const uint32_t *__restrict__ base, const int8_t *__restrict__ digits, const uint32_t *__restrict__ maxlen,
                                  uint32_t *__restrict__ table, uint32_t *__restrict__ out, uint64_t n_items, uint32_t base_stride, uint32_t tw,
                                  const uint32_t *__restrict__ one_rec, const uint32_t *__restrict__ absdelta, int half_dbits,
                                  uint32_t *__restrict__ status);
__global__ void k_decrypt(const uint32_t *__restrict__ cts, const uint32_t *__restrict__ parts, uint32_t n_parts, uint64_t negmask,
                          const uint32_t *__restrict__ ftab, uint32_t *__restrict__ out, uint64_t n_ct, int kbits,
                          const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);
__global__ void k_decrypt3(const uint32_t *__restrict__ cts, const uint32_t *__restrict__ parts, uint32_t n_parts, uint64_t negmask,
                           const uint32_t *__restrict__ ftab, uint32_t *__restrict__ out, uint64_t n_ct, int kbits,
                           const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);

// the latency kernels of wide.hip: one ladder / one composition per wavefront, wavefront-wide layout
__global__ void k_pow_shared_wide(const uint32_t *__restrict__ base, const int8_t *__restrict__ digits, const uint32_t *__restrict__ maxlen,
                                  uint32_t *__restrict__ table, uint32_t *__restrict__ out, uint64_t n_items, uint32_t base_stride, uint32_t tw,
                                  const uint32_t *__restrict__ one_rec, const uint32_t *__restrict__ absdelta, int half_dbits,
                                  uint32_t *__restrict__ status);
__global__ void k_compose_wide(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out, uint64_t n, uint32_t reps,
                               const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status,
                               uint32_t *__restrict__ fallbacks);
__global__ void k_pow_shared_pair(const uint32_t *__restrict__ base, const int8_t *__restrict__ digits, const uint32_t *__restrict__ maxlen,
                                  uint32_t *__restrict__ ring_all, uint32_t *__restrict__ ctl_all, uint32_t *__restrict__ out, uint64_t n_items,
                                  uint32_t base_stride, const uint32_t *__restrict__ one_rec, const uint32_t *__restrict__ absdelta, int half_dbits,
                                  uint32_t *__restrict__ status);
__global__ void k_square_chain_wide(const uint32_t *__restrict__ base, uint32_t *__restrict__ table, uint32_t len,
                                    const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);

// the fixed-base comb (comb.hip, comb.hpp): one level of a table, and the gather fused with the first tree level
__global__ void k_comb_table(uint32_t *__restrict__ table, uint32_t npos, uint32_t w, uint32_t half, const uint32_t *__restrict__ absdelta,
                             int half_dbits, uint32_t *__restrict__ status);
__global__ void k_comb_first(cofhe::CombShape s, const uint32_t *__restrict__ tab0, const uint32_t *__restrict__ tab1,
                             const uint32_t *__restrict__ tabf, const uint32_t *__restrict__ r_exps, const uint32_t *__restrict__ m_exps,
                             const uint32_t *__restrict__ leaf, uint64_t ncols, const uint32_t *__restrict__ one_rec, uint32_t *__restrict__ out,
                             const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);

// ciphertext differences and record inverses (affine.hip): k_add_ct's protocol with the second operand inverted
__global__ void k_sub_ct(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out, uint64_t n_ct,
                         const uint32_t *__restrict__ flag, const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status,
                         uint32_t only);
__global__ void k_sub_ct3(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out, uint64_t n_ct,
                          const uint32_t *__restrict__ flag, const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status,
                          uint32_t only);
__global__ void k_invert_records(const uint32_t *in, uint32_t *out, uint64_t n, uint32_t stride, uint32_t offset);

// the plaintext-left matrix product and matrix Beaver triplets (matmul_left.hip): a rows x cols matrix of `words`-word
// elements transposed (vec16: 16-byte pieces), and out = a . b mod 2^kbits on exponent records (plain_mm.hpp)
__global__ void k_transpose_records(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t rows, uint32_t cols, uint32_t words,
                                    uint32_t vec16);
__global__ void k_plain_matmul(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out, uint32_t n, uint32_t m,
                               uint32_t p, uint32_t kbits);

// the convolution (conv.hip, conv.hpp): level 0 -> 1 of the product tree with its leaves read from the table of the image, and
// the patch matrix n x m written out (vec16: 16-byte pieces); the dense [taps, C, Co] exponent tensor of a grouped
// [taps, C / groups, Co] filter, zero outside the blocks, for the gather route of a convolution with groups
__global__ void k_conv_level0(cofhe::ConvShape s, const uint32_t *__restrict__ table, const uint32_t *__restrict__ one_rec,
                              const uint32_t *__restrict__ ent0, const uint32_t *__restrict__ off_cur, const uint32_t *__restrict__ off_next,
                              const uint32_t *__restrict__ map_next, uint32_t n_next, uint32_t row0, uint32_t rows, uint32_t tw,
                              uint32_t *__restrict__ dst, const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);
__global__ void k_gather_patches(cofhe::ConvShape s, const uint32_t *__restrict__ cts, const uint32_t *__restrict__ one_rec,
                                 uint32_t *__restrict__ out, uint32_t n, uint32_t m, uint32_t vec16);
__global__ void k_expand_group_filters(const uint32_t *__restrict__ w, uint32_t *__restrict__ dense, uint32_t taps, uint32_t C, uint32_t Co,
                                       uint32_t groups, uint32_t vec16);

// the convolution with ciphertext filters and its Beaver triplet (conv_ct.hip, plain_conv.hpp): out = img * w mod 2^kbits on
// exponent records, an implicit GEMM with its left tile read through conv_leaf, and the transposed patch matrix m x n of a
// plaintext image written out, zero records in the padding (vec16: 16-byte pieces)
__global__ void k_plain_conv2d(cofhe::ConvShape s, const uint32_t *__restrict__ img, const uint32_t *__restrict__ w, uint32_t *__restrict__ out,
                               uint32_t kbits);
__global__ void k_gather_patch_exponents(cofhe::ConvShape s, const uint32_t *__restrict__ img, uint32_t *__restrict__ out, uint32_t n, uint32_t m,
                                         uint32_t vec16);

// polynomial evaluation from one opened value (pow_dot.hip; pow_dot.hpp, poly_shift.hpp): out[2e+h] = prod_{i<d} bases[(i n_ct + e) 2 + h]
// ^ exps[i n_ct + e] by one ladder per record whose squarings the d bases share, and the Taylor shift q[i n + e] =
// sum_{j>=i} C(j,i) coef[j] x[e]^(j-i) mod 2^kbits on exponent records, one thread per element
__global__ void k_pow_dot(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ exps, uint32_t *__restrict__ out, uint64_t n_ct, uint32_t d,
                          const uint32_t *__restrict__ one_rec, const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);
__global__ void k_poly_shift(const uint32_t *__restrict__ coef, const uint32_t *__restrict__ x, uint32_t *__restrict__ q, uint64_t n, uint32_t d,
                             uint32_t kbits);

// division by public divisors from one opened value (divide.hip; plain_div.hpp): q[e] = floor(s(v[e]) / div[e mod n_div]) mod
// 2^kbits on exponent records, s the centred residue, one limb group per element
__global__ void k_plain_divfloor(const uint32_t *__restrict__ v, const uint32_t *__restrict__ div, uint64_t n_div, uint32_t *__restrict__ q,
                                 uint64_t n, uint32_t kbits, uint32_t *__restrict__ status);

// exact floor division by small public divisors from one opened value (divide_exact.hip; plain_divmod.hpp): the quotient q[e] and
// the remainder rem[e] in [0, D) of s(v[e]) by D = div[e mod n_div] <= rows, one limb group per element; the blocks prep[e] = q(r[e])
// | q(r[e]) + 1 | (D - m(r[e]), D) of the rows, launched the same way; the plaintext rows out[i rows + j] = q(r_i) + [m(r_i) + j >= D_i]
// for j < D_i and zero records up to rows, stored from those blocks (a grid-stride loop over pieces; vec16: out is 16-byte
// aligned); and the closing copy out[i] = tuples[i rows + index[i]] of ciphertexts (one wavefront per output ciphertext; an index
// of rows or more reads entry 0 and sets CF_ST_DIV_CAP; vec16: tuples and out are 16-byte aligned)
__global__ void k_plain_divmod(const uint32_t *__restrict__ v, const uint32_t *__restrict__ div, uint64_t n_div, uint32_t *__restrict__ q,
                               uint32_t *__restrict__ rem, uint64_t n, uint32_t rows, uint32_t kbits, uint32_t *__restrict__ status);
__global__ void k_divx_prep(const uint32_t *__restrict__ r, const uint32_t *__restrict__ div, uint64_t n_div, uint32_t *__restrict__ prep,
                            uint64_t n, uint32_t rows, uint32_t kbits, uint32_t *__restrict__ status);
__global__ void k_divx_rows(const uint32_t *__restrict__ prep, uint32_t *__restrict__ out, uint64_t n, uint32_t rows, uint32_t vec16);
__global__ void k_divx_select(const uint32_t *__restrict__ index, const uint32_t *__restrict__ tuples, uint32_t *__restrict__ out, uint64_t n,
                              uint32_t rows, uint32_t vec16, uint32_t *__restrict__ status);

// table lookups from one opened value (lut.hip; lut.hpp): the plaintext rows out[i 2^bits + j] = table[(i mod n_tab) 2^bits +
// ((j + r[i]) mod 2^bits)] on exponent records (a grid-stride loop over 16-byte pieces, 8 lanes per record), and the closing copy
// out[i] = tuples[i 2^bits + (e[i] mod 2^bits)] of ciphertexts (one wavefront per output ciphertext); vec16: every table / tuple / out pointer is 16-byte aligned
__global__ void k_lut_rotate(const uint32_t *__restrict__ table, uint64_t n_tab, const uint32_t *__restrict__ r, uint32_t *__restrict__ out,
                             uint64_t n, uint32_t bits, uint32_t vec16);
__global__ void k_lut_select(const uint32_t *__restrict__ e, const uint32_t *__restrict__ tuples, uint32_t *__restrict__ out, uint64_t n,
                             uint32_t bits, uint32_t vec16);

// piecewise-polynomial activations from one opened value (spline.hip; spline.hpp): the plaintext rows out[(i 2^bits + j) (d + 1) + c]
// = coefficient c of the Taylor shift of piece (j + rho_i) mod 2^bits of table i mod n_tab at r_i minus the piece's origin, rho_i =
// bits shift .. shift + bits - 1 of r_i (one thread per element and row); the powers out[(c - 1) n + i] = e[i]^c mod 2^kbits, c = 1
// .. d (one thread per element); and the closing walk out[i] = q_0 o prod_c q_c^powers[(c - 1) n + i] over row j(e[i]) of the
// element's tuple, read in place (one limb group per output record, the walk of k_pow_dot)
__global__ void k_spline_rows(const uint32_t *__restrict__ pieces, uint64_t n_tab, const uint32_t *__restrict__ r, uint32_t *__restrict__ out,
                              uint64_t n, uint32_t bits, uint32_t shift, uint32_t d, uint32_t kbits);
__global__ void k_spline_powers(const uint32_t *__restrict__ e, uint32_t *__restrict__ out, uint64_t n, uint32_t d, uint32_t kbits);
__global__ void k_spline_close(const uint32_t *__restrict__ e, const uint32_t *__restrict__ powers, const uint32_t *__restrict__ tuples,
                               uint32_t *__restrict__ out, uint64_t n, uint32_t bits, uint32_t shift, uint32_t d, uint32_t kbits,
                               const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);

// rearranging resident tensors (view.hip; view.hpp): the box of an affine view, dst[view_dest(i)] = src[view_source(i)] or the fill
// record, and the index gather dst[i] = src[index[i]] with its two sentinels (an index beyond the source: the fill record and
// CF_ST_BAD_INDEX); records of `words` words, one wavefront per record of 64 pieces or more and eight lanes per shorter one;
// vec16: src, fill and dst are 16-byte aligned and words is a multiple of 4
__global__ void k_view_records(cofhe_hip_view v, const uint32_t *__restrict__ src, const uint32_t *__restrict__ fill, uint32_t *__restrict__ dst,
                               uint32_t words, uint32_t vec16);
__global__ void k_gather_records(const uint32_t *__restrict__ src, uint64_t n_src, const uint32_t *__restrict__ index,
                                 const uint32_t *__restrict__ fill, uint32_t *__restrict__ dst, uint64_t n_out, uint32_t words, uint32_t vec16,
                                 uint32_t *__restrict__ status);

// the sign on a window of up to 64 bits from digit comparisons (compare.hip; compare.hpp): the plaintext rows out[(i n + j) 2^d + c]
// = 2^j sgn(r_ij - c) on exponent records, r_ij digit j of r[i] mod 2^bits, n = ceil(bits / d) (pure stores, a grid-stride loop;
// vec16: out is 16-byte aligned), and the closing compositions out[2 i + s] = prod_j tuples[(i n + j) 2^d + digit j of t_s] for
// the two thresholds t_0 = A, t_1 = B of e[i] mod 2^bits, which share the n - 1 factors below the top digit, with wrap[i] = [A > B]
// as an exponent record (one limb group per element and half, n compositions each)
__global__ void k_cmp_rows(const uint32_t *__restrict__ r, uint32_t *__restrict__ out, uint64_t elements, uint32_t bits, uint32_t digit_bits,
                           uint32_t vec16);
__global__ void k_cmp_close(const uint32_t *__restrict__ e, const uint32_t *__restrict__ tuples, uint32_t *__restrict__ out,
                            uint32_t *__restrict__ wrap, uint64_t elements, uint32_t bits, uint32_t digit_bits,
                            const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status);
}  // namespace cofhe_k
