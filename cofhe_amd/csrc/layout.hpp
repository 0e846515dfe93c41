// layout.hpp -- device-resident tensor layout shared by the kernels and the host packer.
//
// A form is one fixed-size record of 168 little-endian u32 words (672 B, 16-byte aligned):
//   words [  0,  40)  a      (magnitude, 1280-bit capacity)
//   words [ 40,  80)  |b|
//   words [ 80, 160)  c      (2560-bit capacity)
//   word   160        1 when b < 0
//   words [161, 168)  zero
// A ciphertext is two consecutive records (c1, c2); a tensor of E ciphertexts is 2E records
// in row-major element order, so the 8 limb groups of a wavefront stream 8 consecutive
// records (5.25 KiB contiguous) and lane gl of a group owns words [5gl, 5gl+5) of every
// 40-word plane -- the register layout of mp.hpp, no shuffles on load.
#pragma once
#include <stdint.h>
namespace cofhe {
constexpr int REC_WORDS = 168;
constexpr int REC_A = 0, REC_B = 40, REC_C = 80, REC_SIGN = 160;

// An op word of the matrix product's schedules (k_matmul_schedule, k_tree_horner_schedule), one composition each:
//   word = kind << 29 | j << 8 | negative << 7 | (|digit| >> 1)
// j has 21 bits: base index < 2^21 (the chains: j < m; the tree's Horner schedule: j = off_T[s] < N_T, see MM_INDEX_LIMIT)
constexpr uint32_t MM_END = 0, MM_SQUARE = 1, MM_MUL = 2, MM_FIRST = 3, MM_ZEROMUL = 4, MM_FIRSTZERO = 5, MM_FIRSTONE = 6;
constexpr uint32_t MM_INDEX_LIMIT = 1u << 21;        // base indices of an op word: 0 .. 2^21 - 1

// Levels of the matrix product's product tree: m < 2^21 entries per segment.  The top level's element index off_T[s] goes
// into the Horner op word's 21-bit base index, so the tree is taken only while N_T <= 2^21 (cofhe_hip_scal_matmul_records;
// N_T reaches ~ len p, not m)
constexpr int TREE_LEVELS = 22;
}  // namespace cofhe
