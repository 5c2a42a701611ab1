// sunscreen_amd/csrc/behzcore.hpp -- per-coefficient BEHZ base conversions (SEAL RNSTool), shared by the
// coefficient-parallel kernels of kernels.hip and the head / tail kernels of kernels_split.hip so that both
// pipelines execute the identical arithmetic.
#pragma once
#include <type_traits>
#include "devarith.hpp"
#include "griddot.hpp"
#include "nttcore.hpp"

namespace hipbfv {

// `asm volatile` uses of wave-uniform doubles: the values must exist (in SGPRs) at this point, so their s_loads cannot be sunk
// into the conditional blocks that consume them
__device__ __forceinline__ void pin_scalar_d(double& v) {
  long long b = __double_as_longlong(v);
  asm volatile("" : "+s"(b));
  v = __longlong_as_double(b);
}
template <int KMAX>
__device__ __forceinline__ void pin_scalars_d(double& a, double (&c)[KMAX], MulOpD& m) {
  pin_scalar_d(a);
#pragma unroll
  for (int i = 0; i < KMAX; i++) pin_scalar_d(c[i]);
  pin_scalar_d(m.w);
  pin_scalar_d(m.wq);
}
#define BEHZ_PIN_SCALARS(a, c, m) \
  do {                            \
    double a_ = (a);              \
    MulOpD m_ = (m);              \
    pin_scalars_d(a_, c, m_);     \
  } while (0)

// fastbconv_m_tilde + sm_mrq for one coefficient: x[i] = residue mod q_i  ->  out[j] = residue mod Bsk_j
// (Evaluator_Multiply steps 1-2, seal_fhe/src/evaluator_base.rs:198-212 -> SEAL bfv_multiply).
template <int KMAX>
__device__ __forceinline__ void behz_extend_coeff(const DevCtx* __restrict__ ctx, const u64 (&x)[KMAX], u64 (&out)[KMAX + 2]) {
  const u32 K = ctx->K, S = ctx->S, KK = ctx->KK;
  u64 y[KMAX];
  u32 rm = 0;
#pragma unroll
  for (int i = 0; i < KMAX; i++) {
    if ((u32)i < K) {
      y[i] = mul_shoup(x[i], ctx->ext_scale[i], ctx->mod[i].q);
      rm += (u32)y[i] * ctx->q_to_mtilde[i];
    }
  }
  rm *= ctx->neg_inv_q_mod_mtilde;  // r_mtilde = -x/q mod 2^32
#pragma unroll
  for (int j = 0; j < KMAX + 2; j++) {
    if ((u32)j < S) {
      const DevMod& pm = ctx->mod[KK + j];
      u128 acc = 0;
#pragma unroll
      for (int i = 0; i < KMAX; i++)
        if ((u32)i < K) acc += (u128)y[i] * ctx->q_to_bsk[j][i];
      u64 rc = rm;
      if (rm >= 0x80000000u) rc += pm.q - 0x100000000ull;  // centred representative
      acc += (u128)rc * ctx->q_mod_bsk[j];
      out[j] = mul_shoup(reduce128_fast(acc, pm), ctx->inv_mtilde_mod_bsk[j], pm.q);
    }
  }
}

// fast_floor (q u Bsk -> Bsk) then Shenoy-Kumaresan (Bsk -> q) for one coefficient.
// y[i]  = x * t * (q/q_i)^{-1} mod q_i (the scaled inverse transform delivers exactly this),
// xb[j] = x * t mod Bsk_j;  out[i] = floor(t*x/q) mod q_i with SEAL's alpha_sk correction.
template <int KMAX>
__device__ __forceinline__ void behz_floor_sk_coeff(const DevCtx* __restrict__ ctx, const u64 (&y)[KMAX], const u64 (&xb)[KMAX + 2],
                                                    u64 (&out)[KMAX]) {
  const u32 K = ctx->K, S = ctx->S, KK = ctx->KK, nB = ctx->nB;
  u64 yb[KMAX + 1];
  u64 fl_msk = 0;
#pragma unroll
  for (int j = 0; j < KMAX + 2; j++) {
    if ((u32)j < S) {
      const DevMod& pm = ctx->mod[KK + j];
      u128 acc = 0;
#pragma unroll
      for (int i = 0; i < KMAX; i++)
        if ((u32)i < K) acc += (u128)y[i] * ctx->q_to_bsk[j][i];
      const u64 conv = reduce128_fast(acc, pm);
      const u64 fl = mul_shoup(xb[j] + pm.q - conv, ctx->inv_q_mod_bsk[j], pm.q);
      if ((u32)j < nB) {
        if (j < KMAX + 1) yb[j < KMAX + 1 ? j : 0] = mul_shoup(fl, ctx->inv_punct_B[j], pm.q);
      } else {
        fl_msk = fl;
      }
    }
  }
  const DevMod& msk = ctx->mod[KK + nB];
  u128 acc = 0;
#pragma unroll
  for (int j = 0; j < KMAX + 1; j++)
    if ((u32)j < nB) acc += (u128)yb[j] * ctx->B_to_msk[j];
  const u64 alpha = mul_shoup(reduce128_fast(acc, msk) + msk.q - fl_msk, ctx->inv_B_mod_msk, msk.q);
  const bool neg = alpha > (msk.q >> 1);
#pragma unroll
  for (int i = 0; i < KMAX; i++) {
    if ((u32)i < K) {
      const DevMod& qm = ctx->mod[i];
      u128 a = 0;
#pragma unroll
      for (int j = 0; j < KMAX + 1; j++)
        if ((u32)j < nB) a += (u128)yb[j] * ctx->B_to_q[i][j];
      if (neg)
        a += (u128)(msk.q - alpha) * ctx->B_mod_q[i];
      else
        a += (u128)alpha * (qm.q - ctx->B_mod_q[i]);
      out[i] = reduce128(a, qm);
    }
  }
}

// ---- the same two conversions in exact FP64 arithmetic (DevCtx::aux_f64: every modulus involved is below 2^50) ----
// Values are integers held in doubles; mul_var / mul_const (ArithD) give |result| <= p*(0.5 + tiny), sums of a
// few such terms stay far below 2^53, so every step is exact.  Where SEAL's result depends on WHICH representative
// of a residue enters a base conversion (the y_i below), the canonical one in [0, p) is formed first.
__device__ __forceinline__ double canonical_d(const ArithD& ar, double v) {
  const double r = ar.reduce(v);
  return r < 0.0 ? r + ar.q : r;
}

// x[i] = canonical residue mod q_i as a double  ->  out[j] = a representative mod Bsk_j with |out[j]| < Bsk_j
template <int KMAX>
__device__ __forceinline__ void behz_extend_coeff_d(const DevCtx* __restrict__ ctx, const double (&x)[KMAX], double (&out)[KMAX + 2]) {
  const u32 K = ctx->K, S = ctx->S, KK = ctx->KK;
  double y[KMAX];
  u32 rm = 0;
#pragma unroll
  for (int i = 0; i < KMAX; i++) {
    if ((u32)i < K) {
      const ArithD ar(ctx->mod[i]);
      double v = ar.mul_const(x[i], ctx->ext_scale_d[i]);
      v = v < 0.0 ? v + ar.q : v;  // mul_const leaves |v| <= q*(0.5 + tiny): canonical after one conditional add
      y[i] = v;
      rm += (u32)ar.to_bits(v) * ctx->q_to_mtilde[i];
    }
  }
  rm *= ctx->neg_inv_q_mod_mtilde;  // r_mtilde = -x/q mod 2^32
  const double rc = (double)(int)rm;  // centred representative in [-2^31, 2^31)
#pragma unroll
  for (int j = 0; j < KMAX + 2; j++) {
    if ((u32)j < S) {
      const ArithD ar(ctx->mod[KK + j]);
      double acc = ar.mul_var(rc, ctx->q_mod_bsk_d[j]);
#pragma unroll
      for (int i = 0; i < KMAX; i++)
        if ((u32)i < K) acc += ar.mul_var(y[i], ctx->q_to_bsk_d[j][i]);
      out[j] = ar.mul_const(ar.reduce(acc), ctx->inv_mtilde_mod_bsk_d[j]);
    }
  }
}

// y[i] = x*t*(q/q_i)^{-1} mod q_i, any representative with |y[i]| < 2^52; xb[j] = x*t mod Bsk_j likewise;
// out[i] = canonical residue (u64) of floor(t*x/q) mod q_i, identical to behz_floor_sk_coeff
template <int KMAX>
__device__ __forceinline__ void behz_floor_sk_coeff_d(const DevCtx* __restrict__ ctx, const double (&y)[KMAX], const double (&xb)[KMAX + 2],
                                                      u64 (&out)[KMAX]) {
  const u32 K = ctx->K, S = ctx->S, KK = ctx->KK, nB = ctx->nB;
  double yc[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; i++)
    if ((u32)i < K) yc[i] = canonical_d(ArithD(ctx->mod[i]), y[i]);
  double yb[KMAX + 1];
  double fl_msk = 0.0;
#pragma unroll
  for (int j = 0; j < KMAX + 2; j++) {
    if ((u32)j < S) {
      const ArithD ar(ctx->mod[KK + j]);
      double conv = 0.0;
#pragma unroll
      for (int i = 0; i < KMAX; i++)
        if ((u32)i < K) conv += ar.mul_var(yc[i], ctx->q_to_bsk_d[j][i]);
      const double fl = ar.mul_const(ar.reduce(ar.reduce(xb[j]) - conv), ctx->inv_q_mod_bsk_d[j]);
      if ((u32)j < nB) {
        if (j < KMAX + 1) yb[j < KMAX + 1 ? j : 0] = canonical_d(ar, ar.mul_const(fl, ctx->inv_punct_B_d[j]));
      } else {
        fl_msk = fl;
      }
    }
  }
  const ArithD am(ctx->mod[KK + nB]);
  double acc = -fl_msk;
#pragma unroll
  for (int j = 0; j < KMAX + 1; j++)
    if ((u32)j < nB) acc += am.mul_var(yb[j], ctx->B_to_msk_d[j]);
  // alpha_sk as the small signed integer it stands for (SEAL branches on alpha_sk > m_sk/2 to the same effect)
  const double alpha = am.reduce(am.mul_const(am.reduce(acc), ctx->inv_B_mod_msk_d));
#pragma unroll
  for (int i = 0; i < KMAX; i++) {
    if ((u32)i < K) {
      const ArithD ar(ctx->mod[i]);
      double a = -ar.mul_var(alpha, ctx->B_mod_q_d[i]);
#pragma unroll
      for (int j = 0; j < KMAX + 1; j++)
        if ((u32)j < nB) a += ar.mul_var(yb[j], ctx->B_to_q_d[i][j]);
      out[i] = ar.canonical(a);
    }
  }
}

// ---- mixed base (DevCtx::aux_mixed): integer-policy data primes (up to 2^56), FP64-policy auxiliary primes (below 2^48) ----
// Every sum whose TARGET is an auxiliary prime runs in exact FP64 like the forms above; a data residue y enters as two
// halves at bit 30, y = yh * 2^30 + yl (yh < 2^32 for any y < 2^62, both exact in a double; the high half meets the constant
// pre-multiplied by 2^30), so a
// K-term sum has 2K products of magnitude <= p/2 each -- far below 2^53.  Sums whose target is a DATA prime (the last step
// of the Shenoy-Kumaresan conversion) stay in 128-bit integers.  Same integers as behz_extend_coeff / behz_floor_sk_coeff.
__device__ __forceinline__ void split30(u64 y, double& hi, double& lo) {
  hi = (double)(u32)(y >> 30);
  lo = (double)(u32)(y & ((1u << 30) - 1u));
}

// x[i] = canonical residue mod q_i (u64)  ->  out[j] = a representative mod Bsk_j with |out[j]| < Bsk_j (double)
template <int KMAX>
__device__ __forceinline__ void behz_extend_coeff_mixed(const DevCtx* __restrict__ ctx, const u64 (&x)[KMAX], double (&out)[KMAX + 2]) {
  const u32 K = ctx->K, S = ctx->S, KK = ctx->KK;
  double yh[KMAX], yl[KMAX];
  u32 rm = 0;
#pragma unroll
  for (int i = 0; i < KMAX; i++) {
    if ((u32)i < K) {
      const u64 y = mul_shoup(x[i], ctx->ext_scale[i], ctx->mod[i].q);
      split30(y, yh[i], yl[i]);
      rm += (u32)y * ctx->q_to_mtilde[i];
    }
  }
  rm *= ctx->neg_inv_q_mod_mtilde;  // r_mtilde = -x/q mod 2^32
  const double rc = (double)(int)rm;  // centred representative in [-2^31, 2^31)
#pragma unroll
  for (int j = 0; j < KMAX + 2; j++) {
    if ((u32)j < S) {
      const ArithD ar(ctx->mod[KK + j]);
      double acc = ar.mul_var(rc, ctx->q_mod_bsk_d[j]);
#pragma unroll
      for (int i = 0; i < KMAX; i++)
        if ((u32)i < K) acc += ar.mul_var(yh[i], ctx->q_to_bsk_hi_d[j][i]) + ar.mul_var(yl[i], ctx->q_to_bsk_d[j][i]);
      out[j] = ar.mul_const(ar.reduce(acc), ctx->inv_mtilde_mod_bsk_d[j]);
    }
  }
}

// y[c][i] = x*t*(q/q_i)^{-1} mod q_i, canonical (u64); xb[c][j] = x*t mod Bsk_j, canonical (u64, below 2^48), for NC
// coefficients c at once (independent chains: the tail kernel takes its four coefficients two at a time);
// out[c][i] = canonical residue of floor(t*x/q) mod q_i, identical to behz_floor_sk_coeff
template <int KMAX, int NC>
__device__ __forceinline__ void behz_floor_sk_coeff_mixed(const DevCtx* __restrict__ ctx, const u64 (&y)[NC][KMAX], const u64 (&xb)[NC][KMAX + 2],
                                                          u64 (&out)[NC][KMAX]) {
  const u32 K = ctx->K, S = ctx->S, KK = ctx->KK, nB = ctx->nB;
  double yh[NC][KMAX], yl[NC][KMAX];
#pragma unroll
  for (int c = 0; c < NC; c++)
#pragma unroll
    for (int i = 0; i < KMAX; i++)
      if ((u32)i < K) split30(y[c][i], yh[c][i], yl[c][i]);
  u64 yb[NC][KMAX + 1];
  const ArithD am(ctx->mod[KK + nB]);
  const double magic = ctx->conv_magic;
  double amsk[NC], fl_msk[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) amsk[c] = 0.0, fl_msk[c] = 0.0;
#pragma unroll
  for (int j = 0; j < KMAX + 2; j++) {
    if ((u32)j < S) {
      const ArithD ar(ctx->mod[KK + j]);
      // the 2K products of the conversion summed exactly on the grid of DevCtx::conv_magic, reduced once (griddot.hpp)
      double hi[NC], lo[NC];
      {
        const double ch = ctx->q_to_bsk_hi_d[j][0];
#pragma unroll
        for (int c = 0; c < NC; c++) {
          const GridDot g(magic, yh[c][0], ch);
          hi[c] = g.acc, lo[c] = g.err;
        }
      }
#pragma unroll
      for (int i = 0; i < KMAX; i++) {
        if ((u32)i < K) {
          const double ch = ctx->q_to_bsk_hi_d[j][i], cl = ctx->q_to_bsk_d[j][i];
#pragma unroll
          for (int c = 0; c < NC; c++) {
            if (i > 0) grid_dot_add(hi[c], lo[c], yh[c][i], ch);
            grid_dot_add(hi[c], lo[c], yl[c][i], cl);
          }
        }
      }
      const MulOpD invq = ctx->inv_q_mod_bsk_d[j];
      double fl[NC];
#pragma unroll
      for (int c = 0; c < NC; c++)
        fl[c] = ar.mul_const(ar.reduce(ArithD::from_u64(xb[c][j]) - (ar.reduce(hi[c] - magic) + lo[c])), invq);
      if ((u32)j < nB) {
        const MulOpD ip = ctx->inv_punct_B_d[j];
        const double bm = ctx->B_to_msk_d[j];
#pragma unroll
        for (int c = 0; c < NC; c++) {
          const double ybd = canonical_d(ar, ar.mul_const(fl[c], ip));
          amsk[c] += am.mul_var(ybd, bm);
          if (j < KMAX + 1) yb[c][j < KMAX + 1 ? j : 0] = ArithD::to_bits(ybd);
        }
      } else {
#pragma unroll
        for (int c = 0; c < NC; c++) fl_msk[c] = fl[c];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NC; c++) {
    // alpha_sk as the signed integer it stands for (SEAL branches on alpha_sk > m_sk/2 to the same effect)
    const double alpha = am.reduce(am.mul_const(am.reduce(amsk[c] - fl_msk[c]), ctx->inv_B_mod_msk_d));
    const bool neg = alpha < 0.0;
    // alpha_sk = e - floor(F / B), e in [0, nB): as large as F / B, i.e. up to m_sk / 4 under the derived base bound (context.cpp;
    // a 32-bit cast here held only while SEAL's sizing kept |F / B| below 2^25 -- the fuzz suite caught it).  An exact integer
    // below 2^48 in magnitude: its bits come out of the double exactly.
    const u64 amag = ArithD::to_bits(neg ? -alpha : alpha);
#pragma unroll
    for (int i = 0; i < KMAX; i++) {
      if ((u32)i < K) {
        const DevMod& qm = ctx->mod[i];
        u128 a = 0;
#pragma unroll
        for (int j = 0; j < KMAX + 1; j++)
          if ((u32)j < nB) a += (u128)yb[c][j] * ctx->B_to_q[i][j];
        // floor = sum - alpha * B: a negative alpha ADDS |alpha| * B, a positive one adds alpha * (q_i - B mod q_i)
        if (neg)
          a += (u128)amag * ctx->B_mod_q[i];
        else
          a += (u128)amag * (qm.q - ctx->B_mod_q[i]);
        out[c][i] = reduce128(a, qm);
      }
    }
  }
}

// ---- the FP64 conversions for NC coefficients at once (the head / tail kernels own 8 / 4 coefficients per thread):
// every base-conversion constant is fetched once and applied to all NC coefficients (NC independent chains), and the
// Shenoy-Kumaresan sums are accumulated as soon as each auxiliary residue is finished, so no per-residue arrays of
// intermediate values stay live.  Same arithmetic, value for value, as the single-coefficient forms above.

// x[i][k]: canonical residue of coefficient k mod q_i (double); ext(j, out): called once per auxiliary prime j with
// out[k] = representative of the extended value mod Bsk_j, |out[k]| < Bsk_j
// GRID: the K + 1 products of each sum formed exactly on the grid of DevCtx::conv_magic and reduced once (griddot.hpp; valid when
// DevCtx::conv_grid == 1: the plan covers K + 1 terms with uncentred constants) -- 4 instructions per term + 5 per sum instead of 7 per term
template <int KMAX, int NC, bool GRID = false, class Sink>
__device__ __forceinline__ void behz_extend_multi_d(const DevCtx* __restrict__ ctx, double (&x)[KMAX][NC], Sink&& ext) {
  const u32 K = ctx->K, S = ctx->S, KK = ctx->KK;
  u32 rm[NC];
#pragma unroll
  for (int k = 0; k < NC; k++) rm[k] = 0;
#pragma unroll
  for (int i = 0; i < KMAX; i++) {
    if ((u32)i < K) {
      const ArithD ar(ctx->mod[i]);
      const MulOpD sc = ctx->ext_scale_d[i];
      const u32 qm = ctx->q_to_mtilde[i];
#pragma unroll
      for (int k = 0; k < NC; k++) {
        double v = ar.mul_const(x[i][k], sc);
        v = v < 0.0 ? v + ar.q : v;
        x[i][k] = v;  // y_i, canonical
        rm[k] += (u32)ArithD::to_bits(v) * qm;
      }
    }
  }
  double rc[NC];
#pragma unroll
  for (int k = 0; k < NC; k++) rc[k] = (double)(int)(rm[k] * ctx->neg_inv_q_mod_mtilde);
#pragma unroll 1
  for (u32 j = 0; j < S; j++) {
    const ArithD ar(ctx->mod[KK + j]);
    double acc[NC];
    // every constant of this auxiliary prime is requested here, unconditionally and together (one scalar-cache round trip per
    // trip of the loop): read inside the `i < K` blocks, each was requested where it was used and waited for on the spot
    const double qmb = ctx->q_mod_bsk_d[j];
    double cj[KMAX];
#pragma unroll
    for (int i = 0; i < KMAX; i++) cj[i] = ctx->q_to_bsk_d[j][i];
    const MulOpD inv = ctx->inv_mtilde_mod_bsk_d[j];
    BEHZ_PIN_SCALARS(qmb, cj, inv);
    if constexpr (GRID) {
      const double magic = ctx->conv_magic;
      // four coefficients at a time: the error accumulators of a group are dead before the next group starts (registers)
      constexpr int GRP = NC < 4 ? NC : 4;
#pragma unroll
      for (int g0 = 0; g0 < NC; g0 += GRP) {
        double hi[GRP], lo[GRP];
#pragma unroll
        for (int k = 0; k < GRP; k++) {
          const GridDot g(magic, rc[g0 + k], qmb);
          hi[k] = g.acc, lo[k] = g.err;
        }
#pragma unroll
        for (int i = 0; i < KMAX; i++) {
          if ((u32)i < K) {
            const double c = cj[i];
#pragma unroll
            for (int k = 0; k < GRP; k++) grid_dot_add(hi[k], lo[k], x[i][g0 + k], c);
          }
        }
#pragma unroll
        for (int k = 0; k < GRP; k++) acc[g0 + k] = ar.mul_const(ar.reduce(ar.reduce(hi[k] - magic) + lo[k]), inv);
      }
    } else {
#pragma unroll
      for (int k = 0; k < NC; k++) acc[k] = ar.mul_var(rc[k], qmb);
#pragma unroll
      for (int i = 0; i < KMAX; i++) {
        if ((u32)i < K) {
          const double c = cj[i];
#pragma unroll
          for (int k = 0; k < NC; k++) acc[k] += ar.mul_var(x[i][k], c);
        }
      }
#pragma unroll
      for (int k = 0; k < NC; k++) acc[k] = ar.mul_const(ar.reduce(acc[k]), inv);
    }
    ext(j, acc);
  }
}

// The mixed-base extension for NC coefficients at once (mul_head owns 8 per thread): the data residues stay packed as two
// 32-bit halves per coefficient (64 registers for K <= 4, NC = 8) and are widened to doubles where a product needs them;
// ext(j, out) is called once per auxiliary prime with out[k] = representative of the extended value, |out[k]| < Bsk_j.
template <int KMAX, int NC, class Sink>
__device__ __forceinline__ void behz_extend_multi_mixed(const DevCtx* __restrict__ ctx, const u64 (&x)[KMAX][NC], Sink&& ext) {
  const u32 K = ctx->K, S = ctx->S, KK = ctx->KK;
  u32 yh[KMAX][NC], yl[KMAX][NC], rm[NC];
#pragma unroll
  for (int k = 0; k < NC; k++) rm[k] = 0;
#pragma unroll
  for (int i = 0; i < KMAX; i++) {
    const MulOp sc = ctx->ext_scale[(u32)i < K ? i : 0];
    const u64 q = ctx->mod[(u32)i < K ? i : 0].q;
    const u32 qm = ctx->q_to_mtilde[(u32)i < K ? i : 0];
#pragma unroll
    for (int k = 0; k < NC; k++) {
      const u64 y = (u32)i < K ? mul_shoup(x[i][k], sc, q) : 0;
      yh[i][k] = (u32)(y >> 30);
      yl[i][k] = (u32)y & ((1u << 30) - 1u);
      rm[k] += (u32)i < K ? (u32)y * qm : 0u;
    }
  }
  double rc[NC];
#pragma unroll
  for (int k = 0; k < NC; k++) rc[k] = (double)(int)(rm[k] * ctx->neg_inv_q_mod_mtilde);
  const double magic = ctx->conv_magic;
#pragma unroll 1
  for (u32 j = 0; j < S; j++) {
    const ArithD ar(ctx->mod[KK + j]);
    // the 2K + 1 products are summed EXACTLY on the grid of DevCtx::conv_magic and reduced once (griddot.hpp: 4 instructions per
    // term + 5 per sum instead of 7 per term)
    double hi[NC], lo[NC];
    const double qmb = ctx->q_mod_bsk_d[j];
#pragma unroll
    for (int k = 0; k < NC; k++) {
      const GridDot g(magic, rc[k], qmb);
      hi[k] = g.acc, lo[k] = g.err;
    }
#pragma unroll
    for (int i = 0; i < KMAX; i++) {
      if ((u32)i < K) {
        const double ch = ctx->q_to_bsk_hi_d[j][i], cl = ctx->q_to_bsk_d[j][i];
#pragma unroll
        for (int k = 0; k < NC; k++) {
          // widened HERE, per auxiliary prime: left to itself the compiler hoists the 2 * K * NC conversions out of the loop
          // and keeps 128 registers of doubles alive across it
          u32 h = yh[i][k], l = yl[i][k];
          asm volatile("" : "+v"(h), "+v"(l));
          grid_dot_add(hi[k], lo[k], (double)h, ch);
          grid_dot_add(hi[k], lo[k], (double)l, cl);
        }
      }
    }
    const MulOpD inv = ctx->inv_mtilde_mod_bsk_d[j];
    double acc[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) acc[k] = ar.mul_const(ar.reduce(ar.reduce(hi[k] - magic) + lo[k]), inv);
    ext(j, acc);
  }
}

// yc[i][k]: CANONICAL y_i of coefficient k (double); finish(j, raw, xb): called once per auxiliary prime j, must fill
// xb[k] = x*t mod Bsk_j (any representative with |xb| < Bsk_j: the K conversion terms of at most 0.875 Bsk_j each are subtracted
// from it as it is -- below 8 Bsk_j < 2^51 at K = 8 -- and the sum reduced once); out[i][k] = canonical u64 result mod q_i
// Two-phase source: fetch(j, raw) only issues the loads of auxiliary residue j (raw words, no arithmetic on them);
// finish(j, raw, xb) turns them into xb.  Residue j+1 is fetched before residue j is consumed, so two residues'
// loads are in flight per thread (the tail kernels are latency-bound, not bandwidth-bound, at their occupancy).
// GRID (DevCtx::conv_grid, used by the 8-prime instantiation): the q -> Bsk sums of the floor are formed exactly on the
// grid of DevCtx::conv_magic and reduced once (griddot.hpp) instead of term by term -- the same residues, so the same
// canonical results.  Measured (interleaved A/B on one box): mul_tail -8.5 % at K = 8 (n = 16384), +1.4 % at K = 4, where a
// sum has too few terms to repay its fixed cost; the same form in the head's extension costs registers (one wave per
// SIMD) for no gain at K = 4 and +8 % at K = 8 (the head is HBM-bound), so the head keeps the per-term reduction.  The
// Shenoy-Kumaresan sums grow across the trips of the loop: in grid form each needs a second loop-carried accumulator and
// the register copies that come with it cancel the saving (ISA count).
// OutT: u64 (canonical words, for a kernel that stores them) or double (the same canonical integers kept as doubles for a fused
// consumer -- the key-switch head's digits, the mod-down's base -- that would convert them straight back: r05)
// ONE_IP: q^-1 and (B/B_j)^-1 as ONE constant product for the primes of B (DevCtx::inv_q_ip_mod_bsk_d) -- the value between the two
// products was used nowhere else; the m_sk row keeps q^-1 alone.  Same canonical y_b (tests/native/tailfold_check.cpp).
template <int KMAX, int NC, bool GRID, bool ONE_IP, class Raw, class Fetch, class Finish, class OutT>
__device__ __forceinline__ void behz_floor_sk_multi_d(const DevCtx* __restrict__ ctx, const double (&yc)[KMAX][NC], Fetch&& fetch, Finish&& finish,
                                                      OutT (&out)[KMAX][NC]) {
  const u32 K = ctx->K, S = ctx->S, KK = ctx->KK, nB = ctx->nB;
  const double magic = GRID ? ctx->conv_magic : 0.0;
  double oacc[KMAX][NC], amsk[NC], flm[NC];
#pragma unroll
  for (int k = 0; k < NC; k++) amsk[k] = 0.0, flm[k] = 0.0;
#pragma unroll
  for (int i = 0; i < KMAX; i++)
#pragma unroll
    for (int k = 0; k < NC; k++) oacc[i][k] = 0.0;
  Raw cur[NC];
  fetch(0u, cur);
#pragma unroll 1
  for (u32 j = 0; j < S; j++) {
    const ArithD ar(ctx->mod[KK + j]);
    Raw nxt[NC];
    fetch(j + 1 < S ? j + 1 : j, nxt);  // the last round re-reads its own residue (cache hit) to keep the loop uniform
    // the constants of this auxiliary prime, requested unconditionally and together at the top of the trip (read inside the
    // `i < K` / `j < nB` blocks, each was requested where it was used and waited for on the spot)
    double cq[KMAX], cb[KMAX];
#pragma unroll
    for (int i = 0; i < KMAX; i++) cq[i] = ctx->q_to_bsk_d[j][i], cb[i] = ctx->B_to_q_d[i][j];
    MulOpD invq = ctx->inv_q_mod_bsk_d[j], ip = ONE_IP ? ctx->inv_q_ip_mod_bsk_d[j] : ctx->inv_punct_B_d[j];
    double bm = ctx->B_to_msk_d[j];
    {
      double unused = 0.0;
      pin_scalars_d(unused, cq, invq);
      pin_scalars_d(bm, cb, ip);
    }
    double fl[NC];
    finish(j, cur, fl);
#pragma unroll
    for (int k = 0; k < NC; k++) cur[k] = nxt[k];
    if constexpr (GRID) {
      double hi[NC], lo[NC];
      {
        const double c = cq[0];
#pragma unroll
        for (int k = 0; k < NC; k++) {
          const GridDot g(magic, yc[0][k], c);
          hi[k] = g.acc, lo[k] = g.err;
        }
      }
#pragma unroll
      for (int i = 1; i < KMAX; i++) {
        if ((u32)i < K) {
          const double c = cq[i];
#pragma unroll
          for (int k = 0; k < NC; k++) grid_dot_add(hi[k], lo[k], yc[i][k], c);
        }
      }
#pragma unroll
      for (int k = 0; k < NC; k++) fl[k] -= ar.reduce(hi[k] - magic) + lo[k];
    } else {
#pragma unroll
      for (int i = 0; i < KMAX; i++) {
        if ((u32)i < K) {
          const double c = cq[i];
#pragma unroll
          for (int k = 0; k < NC; k++) fl[k] -= ar.mul_var(yc[i][k], c);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < NC; k++) fl[k] = ONE_IP ? ar.reduce(fl[k]) : ar.mul_const(ar.reduce(fl[k]), invq);
    if (j < nB) {
      const ArithD am(ctx->mod[KK + nB]);
#pragma unroll
      for (int k = 0; k < NC; k++) {
        fl[k] = canonical_d(ar, ar.mul_const(fl[k], ip));  // yb_j = fl * q^-1 * (B/B_j)^-1, canonical
        amsk[k] += am.mul_var(fl[k], bm);
      }
#pragma unroll
      for (int i = 0; i < KMAX; i++) {
        if ((u32)i < K) {
          const ArithD aq(ctx->mod[i]);
          const double c = cb[i];
#pragma unroll
          for (int k = 0; k < NC; k++) oacc[i][k] += aq.mul_var(fl[k], c);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < NC; k++) flm[k] = ONE_IP ? ar.mul_const(fl[k], invq) : fl[k];
    }
  }
  const ArithD am(ctx->mod[KK + nB]);
  double alpha[NC];
#pragma unroll
  for (int k = 0; k < NC; k++) alpha[k] = am.reduce(am.mul_const(am.reduce(amsk[k] - flm[k]), ctx->inv_B_mod_msk_d));
#pragma unroll
  for (int i = 0; i < KMAX; i++) {
    if ((u32)i < K) {
      const ArithD aq(ctx->mod[i]);
      const double bq = ctx->B_mod_q_d[i];
#pragma unroll
      for (int k = 0; k < NC; k++) {
        const double v = oacc[i][k] - aq.mul_var(alpha[k], bq);
        if constexpr (std::is_same<OutT, double>::value) out[i][k] = canonical_d(aq, v);
        else out[i][k] = aq.canonical(v);
      }
    }
  }
}

}  // namespace hipbfv
