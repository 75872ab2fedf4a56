// What attention.hip (fp32 / fp64) and attention_half.hip (float16 / bfloat16) share: the kernels' parameter block and one call
// as the C ABI entries fill it.  What a call may ask for is checked by attn_route() (attention_route.h), once, before a launcher
// runs; a launcher picks the instantiation and launches.
#pragma once
#include "attention_route.h"
#include "common.h"

#include <atomic>

namespace mvdetr {

struct AttnP {
    int B, H, Sq, Sk, D;
    int64_t q[3], k[3], v[3], o[3], go[3], dq[3], dk[3], dv[3];     // element strides: batch, head, token
    uint32_t thresh;                                                 // dropout: keep iff hash >= thresh
    uint64_t seed;
    double inv_keep;                                                 // 1 / (1 - p)
};

enum class AttnType { f16, bf16, f32, f64 };

struct AttnCall {
    hipStream_t st;
    AttnType type;
    const void *go, *q, *k, *v;             // go: the backward's grad_out
    void *out, *lse;                        // written by the forward, read by the backward
    void *work, *gq, *gk, *gv;
    AttnP p;
    AttnRoute r;
};

// the one entry path (attention.hip)
int attn_entry(AttnEntry entry, AttnCall c, const int64_t *strides, int B, int H, int Sq, int Sk, int D, double dropout_p, uint64_t seed);
// attn_fwd_mfma_half and its forced query tile (attention_half.hip)
int attn_launch_forward_half(const AttnCall &c);
extern std::atomic<int> g_ah_query_tile;

}  // namespace mvdetr
