// The arithmetic of the SCN-LSTM cell's element-wise steps (reference models/scn_cell.py:73-91 and :134-152, the gate of
// models/decoders/attention_scn.py:147-150), used by the kernels of csrc/scn_cell.hip.  Floating-point contraction is off
// inside these functions: every product and sum is rounded where it is written, which fixes the bits of those kernels.
#pragma once
#include "common.h"
#include "kernels.h"

namespace scn {

struct LstmFwdOut { float ig, fg, og, cg, c, tc, h; };
__device__ __forceinline__ LstmFwdOut lstm_fwd_math(float p0, float p1, float p2, float p3, float c_prev) {
#pragma clang fp contract(off)
    LstmFwdOut o;
    o.ig = sigmoidf_(p0); o.fg = sigmoidf_(p1); o.og = sigmoidf_(p2); o.cg = tanhf(p3);
    const float a = o.fg * c_prev, b = o.ig * o.cg;
    o.c = a + b;
    o.tc = tanhf(o.c);
    o.h = o.og * o.tc;
    return o;
}

struct LstmBwdOut { float d0, d1, d2, d3, dc; };
__device__ __forceinline__ LstmBwdOut lstm_bwd_math(float dh, float dcn, float ig, float fg, float og, float cg, float tc,
                                                    float c_prev) {
#pragma clang fp contract(off)
    LstmBwdOut o;
    const float dO = dh * tc;
    const float t2 = tc * tc, om = 1.f - t2;
    const float x = dh * og, y = x * om;
    const float dcc = dcn + y;
    o.d0 = ((dcc * cg) * ig) * (1.f - ig);
    o.d1 = ((dcc * c_prev) * fg) * (1.f - fg);
    o.d2 = (dO * og) * (1.f - og);
    const float c2 = cg * cg;
    o.d3 = (dcc * ig) * (1.f - c2);
    o.dc = dcc * fg;
    return o;
}

__device__ __forceinline__ void mix_bwd_math(float dmx, float dmh, float qx, float qh, float pa, float ph, float& dpx,
                                             float& dph, float& acc_x, float& acc_h) {
#pragma clang fp contract(off)
    dpx = dmx * qx;
    dph = dmh * qh;
    const float a = dmx * pa, b = dmh * ph;
    acc_x = acc_x + a;
    acc_h = acc_h + b;
}

__device__ __forceinline__ void gate_bwd_math(float d, float awe, float g, float& dawe, float& dgpre) {
#pragma clang fp contract(off)
    dawe = d * g;
    dgpre = ((d * awe) * g) * (1.f - g);
}

}  // namespace scn
