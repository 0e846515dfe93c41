// Host build of the index arithmetic of k_view_records (cofhe_amd/csrc/view.hpp): the very functions the kernel calls, driven by
// a plain loop over the elements of the box in the kernel's own index order.  TEST INFRASTRUCTURE ONLY; not linked into the
// product library.
#include "../../cofhe_amd/csrc/view.hpp"

using namespace cofhe;

extern "C" {
int view_sim_descriptor_bytes(void) { return (int)sizeof(cofhe_hip_view); }
// for every element i < n_box of the box: src[i] = the source index, or -1 for the fill record; dst[i] = the destination index
void view_sim_indices(const cofhe_hip_view *v, uint64_t n_box, int64_t *src, uint64_t *dst) {
    for (uint64_t i = 0; i < n_box; i++) {
        uint64_t s = 0;
        src[i] = view_source(*v, i, &s) ? (int64_t)s : -1;
        dst[i] = view_dest(*v, i);
    }
}
// the validator: 0 and the counts, or -1
int view_sim_check(const cofhe_hip_view *v, uint64_t *n_src, uint64_t *n_box, uint64_t *n_dst, int *needs_fill) {
    return view_check(*v, n_src, n_box, n_dst, needs_fill) ? -1 : 0;
}
}
