// The per-step factor record of the bounded TV-LQR (ADMM) kernels, defined once: boxqp.hip reads it at compile time
// (BoxLayout<N, M>), boxqp_values.hip with runtime sizes.  Offsets and sizes in doubles.
#pragma once
#include <hip/hip_runtime.h>

struct BoxRec {
    int oAcl, oK, oMinv, oHinv, oB, oC, oD, oQx, S, SP;
};
constexpr __host__ __device__ BoxRec box_rec_layout(int n, int m) {
    BoxRec r{};
    r.oAcl = 0; r.oK = n * n; r.oMinv = r.oK + m * n; r.oHinv = r.oMinv + m * n; r.oB = r.oHinv + m * m;
    r.oC = r.oB + n * m; r.oD = r.oC + n; r.oQx = r.oD + n; r.S = r.oQx + n;
    r.SP = (r.S + 1) / 2 * 2;               // stride of records in HBM, padded to 16 B
    return r;
}
// records in HBM are staged through an LDS ring of this many slots, two steps ahead of use
constexpr int kBoxRing = 3;
