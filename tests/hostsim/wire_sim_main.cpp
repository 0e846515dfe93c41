// Stand-alone run of the wire-format bodies (wire_sim.cpp) over the width table, for the host sanitizers:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o wire_sim_asan wire_sim_main.cpp wire_sim.cpp
//     ./wire_sim_asan
// Every buffer is a heap block of exactly the size the bodies may touch, so a read or write one byte outside it is reported.
// For each kind: records whose integers take every bit length of their planes (2^(n-1), 2^n - 1 and a pattern with the top bit
// set), of either sign word, are packed, the bytes are unpacked again, and the records must come back (minus zero as +0).
// TEST INFRASTRUCTURE ONLY; tests/test_wire_cpu.py holds the same bodies to the Python model.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

extern "C" {
int wire_sim_rec_words(int kind);
int wire_sim_ints_per_rec(int kind);
uint32_t wire_sim_unpack(const uint8_t *body, const uint64_t *off, uint64_t body_len, uint64_t n_rec, int kind, uint32_t *rec,
                         uint64_t rec_cap_words);
int wire_sim_pack(const uint32_t *rec, uint64_t n_rec, int kind, uint64_t *off, uint8_t *body, uint64_t body_cap, uint64_t *body_len);
}

namespace {
// value `family` of n bits into `words` limbs: 0: 2^(n-1), 1: 2^n - 1, 2: 0xA5 bytes cut to n bits with the top bit set
void put_value(uint32_t *dst, int words, int n, int family) {
    memset(dst, 0, (size_t)words * 4);
    if (n == 0) return;
    if (family != 0) {
        memset(dst, family == 1 ? 0xFF : 0xA5, (size_t)words * 4);
        for (int w = (n + 31) / 32; w < words; w++) dst[w] = 0;
        if (n % 32) dst[(n - 1) / 32] &= (1u << (n % 32)) - 1u;
    }
    dst[(n - 1) / 32] |= 1u << ((n - 1) % 32);
}

int run(int kind) {
    const int rw = wire_sim_rec_words(kind), ipr = wire_sim_ints_per_rec(kind);
    std::vector<uint32_t> rec;
    uint64_t n_rec = 0;
    const int lengths = kind == 0 ? 993 : 2562;
    for (int i = 0; i < lengths; i++)
        for (int family = 0; family < 3; family++)
            for (int sign = 0; sign < (kind == 0 ? 2 : 1); sign++) {
                rec.resize((n_rec + 1) * rw, 0u);
                uint32_t *r = rec.data() + n_rec * rw;
                if (kind == 0) {
                    put_value(r, 31, i, family);
                    r[31] = (uint32_t)sign;
                } else {
                    put_value(r, 40, i % 1280 + 1, family);
                    put_value(r + 40, 40, i % 1281, family);
                    put_value(r + 80, 80, i % 2560 + 1, family);
                    r[160] = (uint32_t)(i / 1281);
                }
                n_rec++;
            }
    if (kind == 2 && n_rec % 2) return 1;
    const uint64_t count = n_rec * ipr;
    // first with no room at all: the length is reported and nothing is packed; then with exactly that much
    uint64_t *off = new uint64_t[count];
    uint64_t need = 0, len = 0;
    uint8_t *none = new uint8_t[1];
    if (wire_sim_pack(rec.data(), n_rec, kind, off, none, 0, &need) != -1 || need == 0) return 2;
    delete[] none;
    uint8_t *body = new uint8_t[need];
    if (wire_sim_pack(rec.data(), n_rec, kind, off, body, need, &len) != 0 || len != need) return 3;
    uint32_t *back = new uint32_t[n_rec * rw];
    const uint32_t err = wire_sim_unpack(body, off, len, n_rec, kind, back, n_rec * rw);
    if (err != 0) return 4;
    int bad = 0;
    for (uint64_t r = 0; r < n_rec && !bad; r++) {
        const uint32_t *a = rec.data() + r * rw, *b = back + r * rw;
        const int sw = kind == 0 ? 31 : 160, mag0 = kind == 0 ? 0 : 40, mag1 = kind == 0 ? 31 : 80;
        bool zero = true;
        for (int w = mag0; w < mag1; w++) zero &= a[w] == 0;
        for (int w = 0; w < rw; w++) {
            const uint32_t want = w == sw ? (a[w] && !zero ? 1u : 0u) : a[w];
            if (b[w] != want) bad = 5;
        }
    }
    printf("kind %d: %llu records, %llu integers, body %llu bytes: %s\n", kind, (unsigned long long)n_rec, (unsigned long long)count,
           (unsigned long long)len, bad ? "MISMATCH" : "ok");
    delete[] off;
    delete[] body;
    delete[] back;
    return bad;
}
}  // namespace

int main() {
    for (int kind = 0; kind <= 2; kind++)
        if (int rc = run(kind)) {
            printf("kind %d failed at step %d\n", kind, rc);
            return 1;
        }
    return 0;
}
