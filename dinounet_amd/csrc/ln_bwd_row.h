// The per-row fp32 arithmetic of the LayerNorm backward, shared by layernorm_bwd_fused_kernel (norm.hip: dy read from global memory) and
// layernorm_bwd_prod_kernel (norm_gemm.hip: dy formed in LDS).  Every operation is written out -- an explicit fma where a product is
// accumulated, contraction switched off for the rest -- so the two kernels compute the same bits from the same inputs.  Left to the
// compiler, which products are contracted into fmas depends on how it pairs the operations of the code around them (it differed from
// element to element inside one kernel), and two kernels with the same source text disagreed in the last bit of isolated dx elements.
#pragma once
#include "common.h"

// one 16-byte vector (VI elements) of a row: xhat, g = dy * w, the row sums' terms and the column sums' terms
template <typename T>
__device__ __forceinline__ void ln_bwd_row_terms(const uint4& rx, const uint4& rg, float mu, float rs, const float (&wv)[Elem<T>::VEC],
                                                 float (&xh)[Elem<T>::VEC], float (&g)[Elem<T>::VEC], float& c1, float& c2,
                                                 float (&sa)[Elem<T>::VEC], float (&sb)[Elem<T>::VEC]) {
#pragma clang fp contract(off)
  constexpr int VI = Elem<T>::VEC;
  const Vec16<T> tx = as_vec<T>(rx);
  const Vec16<T> tg = as_vec<T>(rg);
#pragma unroll
  for (int j = 0; j < VI; j++) {
    const float gy = to_f32(tg.v[j]);
    xh[j] = (to_f32(tx.v[j]) - mu) * rs;
    g[j] = gy * wv[j];
    c1 = c1 + g[j];
    c2 = __builtin_fmaf(g[j], xh[j], c2);
    sa[j] = __builtin_fmaf(gy, xh[j], sa[j]);
    sb[j] = sb[j] + gy;
  }
}

// dx of the same vector: rstd * (g - c1 - xhat * c2) [+ dres]
template <typename T, bool RES>
__device__ __forceinline__ uint4 ln_bwd_row_dx(const float (&xh)[Elem<T>::VEC], const float (&g)[Elem<T>::VEC], float c1, float c2, float rs,
                                               const uint4& rr) {
#pragma clang fp contract(off)
  constexpr int VI = Elem<T>::VEC;
  const Vec16<T> tr = as_vec<T>(rr);
  Vec16<T> o;
#pragma unroll
  for (int j = 0; j < VI; j++) {
    const float t = __builtin_fmaf(-xh[j], c2, g[j] - c1);
    o.v[j] = from_f32<T>(RES ? __builtin_fmaf(rs, t, to_f32(tr.v[j])) : rs * t);
  }
  return as_u4(o);
}
