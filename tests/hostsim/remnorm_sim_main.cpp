// Stand-alone run of the remainder-only long division on the host simulator (remnorm_sim.cpp), for the host sanitizers:
//     g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -o remnorm_sim_asan remnorm_sim_main.cpp remnorm_sim.cpp
//     ./remnorm_sim_asan
// Every record is a heap block of exactly its size.  Numerators and divisors of every length relation the staged numerator has
// an edge at -- divisors of 33, 34, 63..65, 1023..1025, 1044, 1279 and 1280 bits under numerators of the divisor's length up
// to two full planes, as 2^(n-1), 2^n - 1 and a byte pattern with the top bit set -- go through mp_rem_norm and through
// mp_divrem_norm, and the remainders must agree word for word.  (The scratch slice of the simulated group is a member
// of a static struct: an index that leaves the struct is reported, one that stays inside it is not judged here -- the
// static_assert of mp_rem_norm bounds the staged words.)
// TEST INFRASTRUCTURE ONLY; tests/test_remnorm_cpu.py holds the same code to Python integers.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

extern "C" {
int remnorm_sim_run(int op, const uint32_t *in, uint32_t *out, int count);
unsigned remnorm_sim_status(void);
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
}  // namespace

int main() {
    const int dens[] = {33, 34, 63, 64, 65, 1023, 1024, 1025, 1044, 1279, 1280};
    int cases = 0;
    for (int db : dens) {
        const int nums[] = {db - 1, db, db + 1, db + 31, db + 32, db + 33, 1280, 1281, 2 * db < 2560 ? 2 * db : 2560, 2559, 2560};
        for (int nb : nums)
            for (int fn = 0; fn < 3; fn++)
                for (int fd = 0; fd < 3; fd++) {
                    uint32_t *in = new uint32_t[120], *a = new uint32_t[80], *b = new uint32_t[80];
                    put_value(in, 80, nb, fn);
                    put_value(in + 80, 40, db, fd);
                    if (remnorm_sim_run(0, in, a, 1) != 0 || remnorm_sim_run(1, in, b, 1) != 0 || remnorm_sim_status() != 0) return 2;
                    if (memcmp(a, b, 80 * 4) != 0) {
                        printf("mismatch: numerator of %d bits (family %d), divisor of %d bits (family %d)\n", nb, fn, db, fd);
                        return 1;
                    }
                    delete[] in;
                    delete[] a;
                    delete[] b;
                    cases++;
                }
    }
    printf("%d divisions: mp_rem_norm == the remainder of mp_divrem_norm\n", cases);
    return 0;
}
