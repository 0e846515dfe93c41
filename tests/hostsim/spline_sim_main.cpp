// Stand-alone run of the spline's plaintext kernels on the host simulator (spline_sim.cpp), for the host sanitizers:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o spline_sim_asan spline_sim_main.cpp spline_sim.cpp
//     ./spline_sim_asan
// Every buffer is a heap block of exactly its size, so a read or a write beyond a table, a mask, a row or a power is reported.
// For k in {8, 128, 256, 639} (both limb-count paths: the register array and the rows' own output records), degrees 1, 2 and 8,
// windows at the bottom, across a word boundary and at the top of k, and one, three and n tables, every output record must be
// written and reduced (below 2^k, sign word 0), and the index must be the field of the residue that the powers kernel stores as
// the first power.  TEST INFRASTRUCTURE ONLY; tests/test_spline_cpu.py holds the same code to Python integers.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

extern "C" {
int spline_sim_index(const uint32_t *recs, uint64_t n, uint32_t bits, uint32_t shift, uint32_t kbits, uint32_t *idx);
int spline_sim_rows(const uint32_t *pieces, uint64_t n_tab, const uint32_t *r, uint32_t *out, uint64_t n, uint32_t bits, uint32_t shift, uint32_t d,
                    uint32_t kbits);
int spline_sim_powers(const uint32_t *e, uint32_t *out, uint64_t n, uint32_t d, uint32_t kbits);
}

namespace {
uint64_t g_seed = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 7;
    g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 16);
}
// a record of `bits` random magnitude bits and a random sign word
void put_random(uint32_t *rec, uint32_t bits) {
    memset(rec, 0, 32 * 4);
    for (uint32_t l = 0; l < (bits + 31) / 32; l++) rec[l] = rnd();
    if (bits % 32) rec[(bits - 1) / 32] &= (1u << (bits % 32)) - 1u;
    rec[31] = rnd() & 1u;
}
}  // namespace

int main() {
    const uint32_t ks[] = {8, 128, 256, 639}, ds[] = {1, 2, 8};
    int cases = 0;
    for (uint32_t k : ks)
        for (uint32_t d : ds) {
            const uint32_t windows[][2] = {{0, 3}, {30 < k - 4 ? 30u : 1u, 4}, {k - 2, 2}};       // (shift, bits)
            for (const auto &w : windows) {
                const uint32_t t = w[0], b = w[1];
                const uint64_t n = 6, n_tabs[] = {1, 3, n};
                for (uint64_t n_tab : n_tabs) {
                    const uint64_t rows_n = (n << b) * (d + 1);
                    uint32_t *pieces = new uint32_t[(n_tab << b) * (d + 1) * 32], *r = new uint32_t[n * 32], *out = new uint32_t[rows_n * 32];
                    uint32_t *pw = new uint32_t[d * n * 32], *idx = new uint32_t[n];
                    for (uint64_t p = 0; p < (n_tab << b) * (d + 1); p++) put_random(pieces + p * 32, p % 4 ? k : 992);
                    for (uint64_t i = 0; i < n; i++) put_random(r + i * 32, i % 3 ? k : 992);
                    memset(out, 0xA5, rows_n * 32 * 4);
                    memset(pw, 0xA5, d * n * 32 * 4);
                    if (spline_sim_rows(pieces, n_tab, r, out, n, b, t, d, k) != 0 || spline_sim_powers(r, pw, n, d, k) != 0 ||
                        spline_sim_index(r, n, b, t, k, idx) != 0)
                        return 2;
                    // every record written: a value below 2^k, zero words above it, sign word 0
                    for (uint64_t m = 0; m < rows_n + d * n; m++) {
                        const uint32_t *rec = m < rows_n ? out + m * 32 : pw + (m - rows_n) * 32;
                        for (uint32_t l = (k + 31) / 32; l < 32; l++)
                            if (rec[l] != 0) {
                                printf("k = %u, d = %u, window (%u, %u): word %u of record %llu is not zero\n", k, d, t, b, l, (unsigned long long)m);
                                return 1;
                            }
                        if (k % 32 && (rec[(k - 1) / 32] >> (k % 32)) != 0) return 1;
                    }
                    // the powers' first row is the residue of r, whose segment the index is
                    for (uint64_t i = 0; i < n; i++) {
                        const uint32_t *v = pw + i * 32;
                        const uint64_t two = ((uint64_t)(t / 32 + 1 < 32 ? v[t / 32 + 1] : 0) << 32) | v[t / 32];
                        if (((uint32_t)(two >> (t % 32)) & ((1u << b) - 1u)) != idx[i]) {
                            printf("k = %u, window (%u, %u): the index of element %llu is not the field of its residue\n", k, t, b, (unsigned long long)i);
                            return 1;
                        }
                    }
                    delete[] pieces;
                    delete[] r;
                    delete[] out;
                    delete[] pw;
                    delete[] idx;
                    cases++;
                }
            }
        }
    printf("%d cases: rows, powers and indices inside their buffers, every record reduced\n", cases);
    return 0;
}
