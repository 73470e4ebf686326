// odin_cbern.h -- one element of the continuous Bernoulli observation (Loaiza-Ganem & Cunningham 2019;
// ContinuousBernoulliLayer, odin/bay/layers/discrete.py:82-121), shared by the stand-alone kernels of elbo_cbernoulli.hip
// and the fused 1x1 head of pointwise.hip (mode 4).
//
// In logit space, for a logit l and a target t in [0, 1]:
//   log p(t | l) = t l - A(l),   A(l) = log((e^l - 1) / l),  A(0) = 0       (the log-partition)
//   d log p / dl = t - mu(l),    mu = A' = 1 / (1 - e^-l) - 1 / l            (the mean, in (0, 1))
// Two forms, selected per element without a branch:
//   |l| <  CBERN_SWITCH: five-term series  A = l/2 + l^2/24 - l^4/2880 + l^6/181440 - l^8/9676800,
//                                          mu = 1/2 + l/12 - l^3/720 + l^5/30240 - l^7/1209600
//                        (truncation at |l| = 1: 2.1e-9 for A, 2.1e-8 for mu; exact 0 and 1/2 at l = 0)
//   |l| >= CBERN_SWITCH: with a = |l|, e = e^-a, om = 1 - e and R = 1 / (a om)  -- ONE exp, ONE reciprocal, ONE log --
//                          A(a) = a + log(om / a) = a + log(om om R),  A(-a) = A(a) - a = log(om / a)
//                          mu(a) = (a - om) R,                         mu(-a) = 1 - mu(a) = (om - a e) R
//                        (a >= 1: om >= 0.63, a - om >= 0.36, om - a e >= 0.26 -- no cancellation; below the switch the
//                        closed forms lose everything, a = 0 gives 0 * inf, and the select discards them)
// |l| is held at 1e30 inside R so that a om stays a normal float: there log(om / a) is 2^-76 of A.
#pragma once
#include "odin_device.h"

constexpr float CBERN_SWITCH = 1.0f;

// acc += log p(t | l);  g = (mu(l) - t) * sc  (= -sc * d log p / dl)
__device__ __forceinline__ void cbern1(float l, float t, float sc, float& acc, float& g) {
  const float l2 = l * l;
  float As = fmaf(l2, -1.0334160052910053e-7f, 5.5114638447971785e-6f);   // -1/9676800, 1/181440
  As = fmaf(l2, As, -3.4722222222222224e-4f);                              // -1/2880
  As = fmaf(l2, As, 4.1666666666666664e-2f);                               // 1/24
  As = fmaf(l2, As, 0.5f * l);
  float ms = fmaf(l2, -8.2671957671957675e-7f, 3.3068783068783071e-5f);   // -1/1209600, 1/30240
  ms = fmaf(l2, ms, -1.3888888888888889e-3f);                              // -1/720
  ms = fmaf(l2, ms, 8.3333333333333329e-2f);                               // 1/12
  ms = fmaf(l, ms, 0.5f);
  const float a = fabsf(l);
  const float e = odin_exp2(-1.4426950408889634f * a);   // e^-a in [0, 1]
  const float om = 1.f - e;
  const float R = odin_rcp(fminf(a, 1e30f) * om);
  const float Lc = 0.6931471805599453f * odin_log2(om * om * R);       // log(om / a) = A(l) - max(l, 0)
  const float mc = fminf((l >= 0.f ? a - om : om - a * e) * R, 1.f);   // (R carries one ulp: keeps |g| <= sc)
  const bool small = a < CBERN_SWITCH;
  // closed form: t l - max(l, 0) taken as (t - 1) l on the positive side -- t l and l cancel there (t = 1, l = 1e4:
  // log p = 9.2 is half an ulp of 1e4)
  const float tt = (small || l < 0.f) ? t : t - 1.f;
  acc += tt * l - (small ? As : Lc);
  g = ((small ? ms : mc) - t) * sc;
}
