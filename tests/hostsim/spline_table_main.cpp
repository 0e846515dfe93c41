// Stand-alone run of the spline table builder (cofhe_amd/host/spline_table.hpp): prints the table of the logistic sigmoid for
//     spline_table_main BITS SHIFT DEGREE IN_FRAC_BITS OUT_FRAC_BITS
// as "max_error <value>" and one line of DEGREE + 1 integer coefficients per piece.  Needs no GPU, no GMP and no library of the
// project.  TEST INFRASTRUCTURE ONLY; tests/test_spline_cpu.py reads what it prints.
#include <cstdio>
#include <cstdlib>

#include "../../cofhe_amd/host/spline_table.hpp"

int main(int argc, char **argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: %s bits shift degree in_frac_bits out_frac_bits\n", argv[0]);
        return 2;
    }
    uint32_t a[5];
    for (int i = 0; i < 5; i++) a[i] = (uint32_t)strtoul(argv[i + 1], nullptr, 10);
    try {
        const CoFHE::SplineTable t = CoFHE::make_spline_table([](double x) { return 1.0 / (1.0 + std::exp(-x)); }, a[0], a[1], a[2], a[3], a[4]);
        printf("max_error %.17g\n", t.max_error);
        for (uint32_t p = 0; p < (1u << t.bits); p++) {
            for (uint32_t i = 0; i <= t.degree; i++) printf("%lld%c", (long long)t.coef[(size_t)p * (t.degree + 1) + i], i == t.degree ? '\n' : ' ');
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "refused: %s\n", e.what());
        return 1;
    }
    return 0;
}
