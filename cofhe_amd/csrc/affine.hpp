// affine.hpp -- the bodies of the difference kernels (affine.hip), in a header so that the host simulator of the CPU tests
// compiles the very code the kernels run.  The inverse of a reduced form is (a, -b, c), a sign flip (qf_inverse): a - b is
// one composition a o b^-1 where the power b^(2^k - 1) of negate_ciphertext_tensor spends k squarings and a product.
#pragma once
#include "form_io.hpp"

namespace cofhe {

// word route for common factors (qf.hpp), as in the tensor-addition kernels
#ifndef COFHE_ADD_WORD_ROUTE
#define COFHE_ADD_WORD_ROUTE true
#endif

// r = a o b^-1 on form records, the remainder sequence served by the workgroup (every thread of it calls this)
CF_DEV void qf_sub_records(Ctx &c, QForm &r, const uint32_t *a_rec, const uint32_t *b_rec, const QDisc &dd) {
    QForm x, y;
    qf_load(c, x, a_rec);
    qf_load(c, y, b_rec);
    qf_inverse(c, y);
    qf_compose<true, COFHE_ADD_WORD_ROUTE, false>(c, r, x, y, dd);
}

// out = in^-1 on one form record (in == out allowed)
CF_DEV void qf_invert_record(Ctx &c, const uint32_t *in_rec, uint32_t *out_rec) {
    QForm f;
    qf_load(c, f, in_rec);
    qf_inverse(c, f);
    qf_store(c, f, out_rec);
}

}  // namespace cofhe
