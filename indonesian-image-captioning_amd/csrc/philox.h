// Philox4x32-10, the counter-based generator of the sampled rollouts (rollout.hip) and of the augmentation draw (augment.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace scn {

struct u32q { unsigned w[4]; };

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped by the Weyl constants between rounds
__device__ __forceinline__ u32q philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return u32q{{c0, c1, c2, c3}};
}

}  // namespace scn
