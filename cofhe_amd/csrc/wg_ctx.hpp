// wg_ctx.hpp -- the workgroup context of the kernels outside cofhe_hip.hip (comb.hip, affine.hip): 32 limb groups whose
// remainder sequences one wavefront serves (mp.hpp: euclid_run_wg), set up exactly as cofhe_hip.hip's make_wg_ctx does.
#pragma once
#include <hip/hip_runtime.h>

#include "form_io.hpp"

namespace cofhe_k {
constexpr int WG_CTX_LDS_WORDS = cofhe::WG_GROUPS * cofhe::SCRATCH_WORDS + cofhe::WG_MAIL_WORDS;

__device__ __forceinline__ cofhe::Ctx make_served_ctx(uint32_t *lds) {
    using namespace cofhe;
    Ctx c;
    const int lane = (int)(threadIdx.x & 63);
    c.gl = lane & (G - 1);
    c.base4 = (lane & ~(G - 1)) << 2;
    c.scr = lds + (threadIdx.x / G) * SCRATCH_WORDS;
    c.wg_mail = lds + WG_GROUPS * SCRATCH_WORDS;
    c.wg_scr0 = lds;
    c.gi = (int)(threadIdx.x / G);
    c.wave = (int)(((threadIdx.x >> 6) + blockIdx.x) % (WG_BLOCK / 64));
    c.rank = gridDim.x <= NUM_CUS * 4 ? (int)((blockIdx.x / NUM_CUS) & 3u) : -1;
    return c;
}
}  // namespace cofhe_k
