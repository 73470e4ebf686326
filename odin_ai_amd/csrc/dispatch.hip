// dispatch.hip -- which kernel family runs a Conv2D / Conv2DTranspose / Dense op (host code only).
//
// One selector per op walks that op's chain ONCE: the public entry point launches what it returns, a dry run asks it
// for the slab rows, and the odin_*_keeps_range / odin_*_reads_x_range predicates are the selector's answer looked up
// in TRAITS.  The families' own predicates (odin_*_applicable, odin_internal.h) say what a kernel CAN take; the order
// and the extra conditions here say what it DOES take.
#include "odin_device.h"   // (the ODIN_ACT_* constants)
#include "odin_internal.h"

namespace {

enum Family {
  GENERIC,        // the tiled kernels of gather_conv.hip / wgrad.hip: every chain ends here
  SMALLC, PW1X1, SMALLDECONV, SMALLDECONV_GEN,
  FCONV_PLANES, FCONV_RING, FCONV_BLK, CONV5_BLK, TCONV_PLANES, TCONV_RING, TCONV_BLK, IGEMM_H, IGEMM,
  WGRAD_PLANES, WGRAD5_BLK, WGRAD_BLK, IGEMM_H_WGRAD, IGEMM_WGRAD,
  BWD_PLANES, BWD_BLK,   // weight + data gradient of a Conv2DTranspose in one launch
  TCONV_PLANES_FIRST,    // data gradient of the second layer + weight gradient of the first in one launch
  NOT_SERVED,            // an entry point without a generic form declines the geometry
  BWD_PAIR,              // the two gradient calls inside an odin_igemm_pair_begin / _end bracket
  TINY_DENSE, THIN_DENSE, DENSE_H, DENSE_GEMM
};

// THE RANGE CONTRACT (include/odin_hip.h: odin_conv_desc.*_amax) per family.  FOLDS_Y / FOLDS_DX: the family folds
// max|out| into the word it is handed from its own epilogue, as a forward / as a data gradient (every other family is
// followed by ONE absmax pass: keep_range below).  READS_X: as a forward or weight gradient it reads the range word of
// the layer input.
enum { FOLDS_Y = 1, FOLDS_DX = 2, READS_X = 4 };
int traits(Family f) {
  switch (f) {
    case SMALLC: case SMALLDECONV_GEN: return FOLDS_Y;
    case SMALLDECONV: case IGEMM: case THIN_DENSE: return FOLDS_Y | FOLDS_DX;
    case FCONV_PLANES: case FCONV_BLK: case CONV5_BLK: case TCONV_PLANES: case TCONV_BLK: case IGEMM_H: case DENSE_H:
      return FOLDS_Y | FOLDS_DX | READS_X;
    case WGRAD_PLANES: case WGRAD5_BLK: case WGRAD_BLK: case IGEMM_H_WGRAD: return READS_X;
    case BWD_PLANES: case BWD_BLK: case DENSE_GEMM: case TCONV_PLANES_FIRST: return FOLDS_DX;
    default: return 0;   // generic gather, 1x1 stream kernel, the fp32 ring kernels, tiny Dense
  }
}

// A tensor that is handed a word leaves a valid bound in it, whatever family ran.  Round 4 left the words of the
// non-folding families untouched and told the caller through the *_keeps_range predicates -- a predicate that disagreed
// with the dispatch (a column-sum slab sends a layer of > ODIN_MAX_COLSUM_BLOCKS tiles to the generic kernel) handed the
// consumers a ZERO word: they scaled by 2^115 and overflowed.  The predicates remain as "kept without an extra pass".
int keep_range(int rc, Family f, int fold_bit, const float* t, size_t n, uint32_t* word, void* stream) {
  if (rc != 0 || t == nullptr || word == nullptr || (traits(f) & fold_bit)) return rc;
  return odin_absmax_fold(t, n, word, stream);
}

bool doubles(const odin_geom& g) { return g.OH == 2 * g.H && g.OW == 2 * g.W; }
bool same_size(const odin_geom& g) { return g.H == g.OH && g.W == g.OW; }
bool aligned16(const void* a, const void* b, const void* c, const void* d) {
  return ((((size_t)a | (size_t)b | (size_t)c | (size_t)d)) & 15) == 0;
}

// ---- selectors: l = the layer's forward gather, g = the gather of the op itself -------------------------------------

Family select_conv2d_fwd(const odin_geom& g, bool bias, int act) {
  if (odin_smallc_applicable(g)) return SMALLC;
  if (odin_pw1x1_applicable(g)) return PW1X1;
  if (act == ODIN_ACT_ELU && bias && odin_fconv_planes_applicable(g)) return FCONV_PLANES;
  if (act == ODIN_ACT_ELU && bias && odin_fconv_ring_applicable(g)) return FCONV_RING;
  // 5x5 / stride-1 layers (the MNIST conv stack): block windows with the weights in LDS (blk5_planes.hip)
  if (bias && same_size(g) && odin_conv5_blk_applicable(g)) return CONV5_BLK;
  if (bias && odin_fconv_blk_applicable(g)) return FCONV_BLK;
  if (odin_igemm_h_applicable(0, g)) return IGEMM_H;
  if (odin_igemm_applicable(0, g)) return IGEMM;
  return GENERIC;
}

// the fp32 implicit GEMM writes one column-sum row per tile: with a slab (or in a dry run, which sizes one) only up to
// ODIN_MAX_COLSUM_BLOCKS tiles
bool igemm_dgrad(int tmode, const odin_geom& g, bool slab, bool dry) {
  return odin_igemm_applicable(tmode, g) && (odin_igemm_tiles(tmode, g) <= ODIN_MAX_COLSUM_BLOCKS || (!slab && !dry));
}

// data gradient of a Conv2D = transposed gather over dY: input (OH, OW, Cout), output (H, W, Cin).  aux_ok: the aux
// tensor is there (or a dry run cannot tell)
Family select_conv2d_dgrad(const odin_geom& l, const odin_geom& g, int aux_act, bool aux_ok, bool slab, bool dry) {
  if (odin_pw1x1_applicable(l)) return PW1X1;
  if (aux_act == ODIN_ACT_ELU && aux_ok && doubles(g) && odin_tconv_planes_applicable(g, 2, 1)) return TCONV_PLANES;
  if (aux_act == ODIN_ACT_ELU && aux_ok && doubles(g) && odin_tconv_ring_applicable(g)) return TCONV_RING;
  if (same_size(g) && odin_conv5_blk_applicable(g)) return CONV5_BLK;
  // any other image size: 8 x 8 blocks of dy through LDS windows (blk_planes.hip)
  if (doubles(g) && odin_tconv_blk_applicable(g)) return TCONV_BLK;
  if (odin_igemm_h_applicable(1, g)) return IGEMM_H;
  if (igemm_dgrad(1, g, slab, dry)) return IGEMM;
  return GENERIC;
}

// the same data gradient, taking the weight gradient of the layer below (l0: its forward gather, the FIRST layer of the
// stack) with it: one family, and no generic form -- the caller keeps the two calls
Family select_conv2d_dgrad_first(const odin_geom& l, const odin_geom& g, const odin_geom& l0, int aux_act, bool aux_ok) {
  if (select_conv2d_dgrad(l, g, aux_act, aux_ok, false, false) != TCONV_PLANES) return NOT_SERVED;
  return odin_tconv_planes_first_applicable(g, l0) ? TCONV_PLANES_FIRST : NOT_SERVED;
}

Family select_deconv2d_fwd(const odin_geom& g, bool bias, int act) {
  if (bias && odin_smalldeconv_applicable(g)) return SMALLDECONV;
  if (act == ODIN_ACT_ELU && bias && doubles(g) && odin_tconv_planes_applicable(g, 1, 1)) return TCONV_PLANES;
  if (act == ODIN_ACT_ELU && bias && doubles(g) && odin_tconv_ring_applicable(g)) return TCONV_RING;
  // a thin small image the implicit-GEMM families cannot take (fewer than 8 channels: MNIST's first deconvolution)
  if (bias && (g.CI & 7) != 0 && odin_smalldeconv_gen_applicable(g)) return SMALLDECONV_GEN;
  if (bias && doubles(g) && odin_tconv_blk_applicable(g)) return TCONV_BLK;
  if (odin_igemm_h_applicable(1, g)) return IGEMM_H;
  if (odin_igemm_applicable(1, g)) return IGEMM;
  return GENERIC;
}

// data gradient of a Conv2DTranspose = strided gather over dY: input (OH, OW, Cout), output (H, W, Cin)
Family select_deconv2d_dgrad(const odin_geom& l, const odin_geom& g, int aux_act, bool aux_ok, bool slab, bool dry) {
  if (!slab && odin_smalldeconv_applicable(l)) return SMALLDECONV;
  if (aux_act == ODIN_ACT_ELU && aux_ok && odin_fconv_planes_applicable(g)) return FCONV_PLANES;
  if (odin_fconv_blk_applicable(g)) return FCONV_BLK;
  if (odin_igemm_h_applicable(0, g)) return IGEMM_H;
  // (64 reduction channels take two fconv_ring passes: where the implicit-GEMM kernel covers the layer it does the
  // same work in one launch -- decoder2 of the dSprites stack: 30.8 us in two launches vs 30.2 us in one)
  const bool ring_two_pass_vs_igemm =
      g.CI == 64 && odin_igemm_applicable(0, g) && odin_igemm_tiles(0, g) <= ODIN_MAX_COLSUM_BLOCKS;
  if (!ring_two_pass_vs_igemm && aux_act == ODIN_ACT_ELU && aux_ok && odin_fconv_ring_applicable(g)) return FCONV_RING;
  if (igemm_dgrad(0, g, slab, dry)) return IGEMM;
  return GENERIC;
}

Family select_bernoulli_tail(int is_deconv, const odin_geom& g, int act, int C1) {
  if (is_deconv && act == ODIN_ACT_ELU && doubles(g) && odin_tconv_planes_applicable(g, 3, C1)) return TCONV_PLANES;
  if (is_deconv && act == ODIN_ACT_ELU && g.CO == 32 && (C1 == 1 || C1 == 3) && doubles(g) &&
      odin_tconv_ring_applicable(g))
    return TCONV_RING;
  return GENERIC;
}

// weight gradients: g.H/W/CI = the fine operand, g.OH/OW/CO = the coarse one.  The part of the chain every layer kind
// shares (a Dense layer that no Dense family takes walks it as a 1x1 convolution).
Family select_wgrad_shared(const odin_geom& g, bool want_bias) {
  if (odin_wgrad_planes_applicable(g)) return WGRAD_PLANES;
  if (same_size(g) && want_bias && odin_wgrad5_blk_applicable(g)) return WGRAD5_BLK;
  if (odin_wgrad_blk_applicable(g)) return WGRAD_BLK;
  if (odin_igemm_h_wgrad_applicable(g)) return IGEMM_H_WGRAD;
  if (odin_igemm_wgrad_applicable(g)) return IGEMM_WGRAD;
  return GENERIC;
}
Family select_conv2d_wgrad(const odin_geom& g) {
  if (odin_smallc_applicable(g)) return SMALLC;
  if (odin_pw1x1_applicable(g)) return PW1X1;
  return select_wgrad_shared(g, true);
}
// (fine operand = dy, coarse = x: g is the data-gradient gather; no bias row)
Family select_deconv2d_wgrad(const odin_geom& l, const odin_geom& g) {
  if (odin_smalldeconv_applicable(l)) return SMALLDECONV;
  return select_wgrad_shared(g, false);
}

// both: dx and wslab are asked for; a dry run (neither) reports the rows of the ONE-call form: with 64 output channels
// the fused launch writes more slab rows than odin_deconv2d_wgrad alone; callers size their slab for both
Family select_deconv2d_bwd(const odin_geom& l, const odin_geom& g, int aux_act, bool aux, bool both, bool dry,
                           bool slab) {
  // the decoders' first Conv2DTranspose: weight and data gradient in ONE launch that stages dy once (smalldeconv.hip)
  if (!slab && both && odin_smalldeconv_applicable(l)) return SMALLDECONV;
  const bool k4s2 = l.KH == 4 && l.KW == 4 && l.S == 2 && l.pt == 1 && l.pl == 1 && doubles(l);
  // dy is fetched, scaled and split ONCE for both gradients (bwd_planes.hip); with 32 output channels the same
  // partial sums as the two launches
  if (((both && aux) || dry) && aux_act == ODIN_ACT_ELU && k4s2 && odin_bwd_planes_applicable(l) &&
      odin_wgrad_planes_applicable(g) && odin_fconv_planes_applicable(g))
    return BWD_PLANES;
  // any other image size: the block-window form of the same launch (blk_planes.hip), 32 output channels
  if ((both || dry) && k4s2 && !l.center && odin_bwd_blk_applicable(l)) return BWD_BLK;
  return BWD_PAIR;
}

// Dense layers whose reduction width is a multiple of 8 through the implicit-GEMM kernel (a 1x1 convolution on a
// 1x1 image; FactorVAE's 1000-unit discriminator, the 512-unit default nets; enc4 of the dSprites step:
// 12.6 + 9.2 + 7.7 -> 9.9 + 9.6 + 6.4 us stand-alone, 11 us per step in the graph); ODIN_NODENSEIGEMM: A/B switch
bool dense_via_igemm() { return ODIN_DIAG_ENV("ODIN_NODENSEIGEMM") == nullptr; }

// aligned: every pointer of the call is 16-byte aligned (the thin streaming kernels need it)
Family select_dense_fwd(int B, int K, int N, bool aligned) {
  if (odin_tiny_dense_ok(B, K, N)) return TINY_DENSE;
  // one thin side (FactorVAE's first / last discriminator layers): streaming kernels, range word kept by the kernel
  if (odin_thin_dense_kind(B, K, N) != 0 && aligned) return THIN_DENSE;
  if (odin_dense_h_ok(B, K, N)) return DENSE_H;
  if (dense_via_igemm() && odin_igemm_applicable(0, odin_geom_dense(B, K, N))) return IGEMM;
  if (odin_dense_gemm_ok(B, K, N)) return DENSE_GEMM;
  return GENERIC;
}
// (only the tiny and the generic kernels write a column-sum slab)
Family select_dense_dgrad(int B, int K, int N, bool slab, bool aligned) {
  if (odin_tiny_dense_ok(B, K, N)) return TINY_DENSE;
  if (slab) return GENERIC;
  if (odin_thin_dense_kind(B, K, N) != 0 && aligned) return THIN_DENSE;
  if (odin_dense_h_ok(B, K, N)) return DENSE_H;
  // (as a transposed 1x1 gather: reduction over the N outputs, weights [k_in][n] with n contiguous)
  if (dense_via_igemm() && odin_igemm_applicable(1, odin_geom_dense(B, N, K))) return IGEMM;
  if (odin_dense_gemm_ok(B, K, N)) return DENSE_GEMM;
  return GENERIC;
}
// aligned: as above, or a dry run (it cannot see the pointers: callers allocate at least 16-byte aligned tensors)
Family select_dense_wgrad(int B, int K, int N, bool aligned) {
  if (odin_dense_h_ok(B, K, N)) return DENSE_H;   // both widths >= 256: the two-plane GEMM, ONE complete slab row
  // one thin side: streaming kernel, slab rows = row chunks of the batch
  if (odin_thin_dense_wgrad_rows(B, K, N) > 0 && aligned) return THIN_DENSE;
  // (also the tiny layers: their forward / data gradient run on the vector ALUs, but the weight gradient
  // through the generic kernel was a 14.5 us launch for 0.001 GFLOP)
  if (dense_via_igemm() && !odin_tiny_dense_ok(B, K, N) && odin_igemm_wgrad_applicable(odin_geom_dense(B, K, N)))
    return IGEMM_WGRAD;
  // small GEMM: the waves of a workgroup split the batch, the result is complete: ONE slab row
  if (odin_dense_gemm_ok(B, K, N) && !ODIN_DIAG_ENV("ODIN_NOTINYWGRADGEMM")) return DENSE_GEMM;
  return select_wgrad_shared(odin_geom_dense(B, K, N), true);
}
Family select_dense_bwd(int B, int K, int N, bool slab) {
  return odin_dense_h_ok(B, K, N) && !slab ? DENSE_H : BWD_PAIR;
}

// ---- launches shared by the ops ------------------------------------------------------------------------------------

// one gather through the families any chain may pick: epi 1 = forward (bias + act), epi 2 = data gradient (x act'(aux),
// column sums into colsum); tmode: transposed gather, wmode: weight layout of the generic kernel
int launch_gather(Family f, int tmode, int wmode, const odin_geom& g, const float* in, const float* w, const float* bias,
                  const float* aux, int aux_act, float* out, float* colsum, int* rows_out, int epi, int act,
                  const uint32_t* in_amax, uint32_t* out_amax, void* stream) {
  const float* blk_aux = aux_act != 0 ? aux : nullptr;
  const int blk_act = epi == 1 ? act : aux_act;
  switch (f) {
    case FCONV_PLANES:
      return odin_fconv_planes_launch(in, w, bias, aux, out, colsum, rows_out, g.B, g.OH, g.OW, g.CI, g.CO, epi, in_amax,
                                      out_amax, stream);
    case FCONV_RING:
      return odin_fconv_ring_launch(in, w, bias, aux, out, colsum, rows_out, g.B, g.H, g.W, g.CI, g.OH, g.OW, g.CO, epi,
                                    stream);
    case FCONV_BLK:
      return odin_fconv_blk_launch(in, w, bias, blk_aux, out, colsum, rows_out, g.B, g.OH, g.OW, g.CI, g.CO, epi, blk_act,
                                   in_amax, out_amax, stream);
    case CONV5_BLK:
      return odin_conv5_blk_launch(in, w, bias, blk_aux, out, colsum, rows_out, g.B, g.H, g.W, g.CI, g.CO, g.KH, epi,
                                   blk_act, in_amax, out_amax, stream);
    case TCONV_PLANES:
      return odin_tconv_planes_launch(in, w, bias, aux, out, colsum, rows_out, nullptr, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, 1, g.B, g.H, g.W, g.CI, g.CO, epi, in_amax, out_amax, stream);
    case TCONV_RING:
      return odin_tconv_ring_launch(in, w, bias, aux, out, colsum, rows_out, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, 1, g.B, g.H, g.W, g.CO, epi, stream);
    case TCONV_BLK:
      return odin_tconv_blk_launch(in, w, bias, blk_aux, out, colsum, rows_out, g.B, g.H, g.W, g.CI, g.CO, epi, blk_act,
                                   in_amax, out_amax, stream);
    case IGEMM_H:
      return odin_igemm_h_launch(tmode, in, w, bias, aux, aux_act, out, colsum, g.B, g.H, g.W, g.CI, g.OH, g.OW, g.CO, g.KH,
                                 g.KW, g.S, g.pt, g.pl, act, in_amax, epi == 2, out_amax, stream);
    case IGEMM:
      return odin_igemm_launch(tmode, in, w, bias, aux, aux_act, out, colsum, g.B, g.H, g.W, g.CI, g.OH, g.OW, g.CO, g.KH,
                               g.KW, g.S, g.pt, g.pl, act, out_amax, stream);
    default:
      return odin_gather_generic(tmode, wmode, g, in, w, bias, act, aux, aux_act, out, colsum,
                                 colsum ? -ODIN_MAX_COLSUM_BLOCKS : odin_num_cus(), rows_out, nullptr, nullptr, stream);
  }
}

// column-sum rows of a data gradient, for the families that do not plan their grid at launch (< 0: the launch reports them)
int dgrad_rows(Family f, int tmode, const odin_geom& g) {
  switch (f) {
    case SMALLDECONV: return 0;
    case IGEMM_H: return odin_igemm_h_rows(tmode, g);
    case IGEMM: return odin_igemm_tiles(tmode, g);
    default: return -1;
  }
}

int conv_dgrad(Family f, int tmode, int wmode, const odin_geom& g, const float* dy, const float* w, const float* aux,
               int aux_act, float* dx, float* colsum_slab, int* slab_rows_out, const odin_conv_desc* d, void* stream) {
  const int rows = dgrad_rows(f, tmode, g);
  if (rows >= 0) {
    if (slab_rows_out) *slab_rows_out = rows;
    if (dx == nullptr) return 0;  // dry run
  }
  int rc;
  if (f == PW1X1) rc = odin_pw1x1_dgrad(dy, w, aux, aux_act, dx, colsum_slab, slab_rows_out, d, stream);
  else if (f == SMALLDECONV) rc = odin_smalldeconv_bwd(nullptr, dy, w, aux, aux_act, dx, nullptr, nullptr, d, stream);
  else
    rc = launch_gather(f, tmode, wmode, g, dy, w, nullptr, aux, aux_act, dx, colsum_slab, slab_rows_out, 2, 0, d->dy_amax,
                       d->dx_amax, stream);
  return keep_range(rc, f, FOLDS_DX, dx, (size_t)d->B * d->H * d->W * d->Cin, d->dx_amax, stream);
}

int conv_fwd(Family f, int tmode, int wmode, const odin_geom& g, const float* x, const float* w, const float* bias,
             float* y, const odin_conv_desc* d, void* stream) {
  int rc;
  switch (f) {
    case SMALLC: rc = odin_smallc_fwd(x, w, bias, y, d, stream); break;
    case PW1X1: rc = odin_pw1x1_fwd(x, w, bias, y, d, stream); break;
    case SMALLDECONV: rc = odin_smalldeconv_fwd(x, w, bias, y, d, stream); break;
    case SMALLDECONV_GEN: rc = odin_smalldeconv_gen_fwd(x, w, bias, y, d, stream); break;
    default:
      rc = launch_gather(f, tmode, wmode, g, x, w, bias, nullptr, 0, y, nullptr, nullptr, 1, d->act, d->x_amax, d->y_amax,
                         stream);
  }
  return keep_range(rc, f, FOLDS_Y, y, (size_t)d->B * d->OH * d->OW * d->Cout, d->y_amax, stream);
}

// the shared weight-gradient families: in / dy = the fine / coarse operand; g_amax / a_amax: range words of the gradient
// and the activation operand (whichever side they are on: grad_u = the fine operand is the gradient)
int launch_wgrad(Family f, const odin_geom& g, const float* in, const float* dy, float* slab, int want_bias,
                 const uint32_t* g_amax, const uint32_t* a_amax, int* rows_out, void* stream) {
  const int grad_u = want_bias ? 0 : 1;
  const int slab_stride = g.KH * g.KW * g.CI * g.CO + (want_bias ? g.CO : 0);
  if (f == IGEMM_H_WGRAD || f == IGEMM_WGRAD) {
    if (rows_out) *rows_out = f == IGEMM_H_WGRAD ? odin_igemm_h_wgrad_rows(g) : odin_igemm_wgrad_rows(g);
    if (slab == nullptr) return 0;  // dry run
  }
  switch (f) {
    case WGRAD_PLANES:
      return odin_wgrad_planes_launch(in, dy, slab, rows_out, g.B, g.OH, g.OW, g.CI, g.CO, want_bias, grad_u, g_amax, a_amax,
                                      stream);
    case WGRAD5_BLK:
      return odin_wgrad5_blk_launch(in, dy, slab, rows_out, g.B, g.H, g.W, g.CI, g.CO, g.KH, want_bias, g_amax, a_amax,
                                    stream);
    case WGRAD_BLK:
      return odin_wgrad_blk_launch(in, dy, slab, rows_out, g.B, g.OH, g.OW, g.CI, g.CO, want_bias, grad_u, g_amax, a_amax,
                                   stream);
    case IGEMM_H_WGRAD:
      return odin_igemm_h_wgrad_launch(in, dy, slab, slab_stride, g.B, g.H, g.W, g.CI, g.OH, g.OW, g.CO, g.KH, g.KW, g.S,
                                       g.pt, g.pl, want_bias, grad_u, g_amax, a_amax, stream);
    case IGEMM_WGRAD:
      return odin_igemm_wgrad_launch(in, dy, slab, slab_stride, g.B, g.H, g.W, g.CI, g.OH, g.OW, g.CO, g.KH, g.KW, g.S, g.pt,
                                     g.pl, want_bias, stream);
    default:
      return odin_wgrad_generic(g, in, dy, slab, want_bias, rows_out, stream);
  }
}

// the two gradient calls of a *_bwd entry point ran inside an odin_igemm_pair_begin bracket: close it
int pair_end(int rc) {
  const int rc2 = odin_igemm_pair_end();
  return rc != 0 ? rc : rc2;
}

}  // namespace

// ---- Conv2D -------------------------------------------------------------------------------------------------------
extern "C" int odin_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, const odin_conv_desc* d,
                               void* stream) {
  const odin_geom g = odin_geom_fwd(d);
  return conv_fwd(select_conv2d_fwd(g, bias != nullptr, d->act), 0, 0, g, x, w, bias, y, d, stream);
}

// dx[b,ih,iw,ci] = sum_{kh,kw,co} dy[b,(ih+pt-kh)/S,(iw+pl-kw)/S,co] * W[kh,kw,ci,co];
// optionally multiplied by act'(aux) (aux = this layer's input = previous layer's output)
extern "C" int odin_conv2d_dgrad(const float* dy, const float* w, const float* aux, int aux_act, float* dx,
                                 float* colsum_slab, int* slab_rows_out, const odin_conv_desc* d, void* stream) {
  const odin_geom g = odin_geom_dgrad(d);
  const Family f = select_conv2d_dgrad(odin_geom_fwd(d), g, aux_act, aux != nullptr || dx == nullptr,
                                       colsum_slab != nullptr, dx == nullptr);
  return conv_dgrad(f, 1, 1, g, dy, w, aux, aux_act, dx, colsum_slab, slab_rows_out, d, stream);
}

extern "C" int odin_conv2d_wgrad(const float* x, const float* dy, float* slab, int* slab_rows_out,
                                 const odin_conv_desc* d, void* stream) {
  const odin_geom g = odin_geom_fwd(d);
  const Family f = select_conv2d_wgrad(g);
  if (f == SMALLC) return odin_smallc_wgrad(x, dy, slab, slab_rows_out, d, stream);
  if (f == PW1X1) return odin_pw1x1_wgrad(x, dy, slab, slab_rows_out, d, stream);
  return launch_wgrad(f, g, x, dy, slab, 1, d->dy_amax, d->x_amax, slab_rows_out, stream);
}

// ---- a layer's whole backward pass in one call: weight gradient + data gradient.  Where both run on the
// implicit-GEMM kernels (igemm.hip) they share ONE launch; otherwise exactly the two calls. ----
extern "C" int odin_conv2d_bwd(const float* x, const float* dy, const float* w, const float* aux, int aux_act, float* dx,
                               float* colsum_slab, int* colsum_rows_out, float* wslab, int* wslab_rows_out,
                               const odin_conv_desc* d, void* stream) {
  odin_igemm_pair_begin();
  int rc = odin_conv2d_wgrad(x, dy, wslab, wslab_rows_out, d, stream);
  if (rc == 0) rc = odin_conv2d_dgrad(dy, w, aux, aux_act, dx, colsum_slab, colsum_rows_out, d, stream);
  return pair_end(rc);
}

// The data gradient of layer d (the SECOND layer) and the weight gradient of the layer below it (d0, the FIRST layer
// of the stack, input x0) in one launch: dx never has to reach memory (dx == NULL: not stored); colsum_slab (optional) as
// in odin_conv2d_dgrad, one row per slab row.  wslab0 == NULL: dry run.
extern "C" int odin_conv2d_dgrad_first(const float* dy, const float* w, const float* aux, int aux_act, float* dx,
                                       float* colsum_slab, int* colsum_rows_out, const odin_conv_desc* d, const float* x0,
                                       float* wslab0, int* wslab0_rows_out, const odin_conv_desc* d0, void* stream) {
  const bool dry = wslab0 == nullptr;
  const Family f = select_conv2d_dgrad_first(odin_geom_fwd(d), odin_geom_dgrad(d), odin_geom_fwd(d0), aux_act,
                                             aux != nullptr || dry);
  if (f != TCONV_PLANES_FIRST) return odin_fail(-2, "conv2d_dgrad_first: shapes outside the kernel");
  if (!dry && (dy == nullptr || w == nullptr || x0 == nullptr))
    return odin_fail(-2, "conv2d_dgrad_first: null argument");
  int rows = 0;
  const int rc = odin_tconv_planes_first_launch(dy, w, aux, dx, colsum_slab, x0, d0->center, wslab0, &rows, d->B, d->dy_amax,
                                                d->dx_amax, stream);
  if (rc == 0 && wslab0_rows_out) *wslab0_rows_out = rows;
  if (rc == 0 && colsum_rows_out) *colsum_rows_out = rows;
  return keep_range(rc, f, FOLDS_DX, dx, (size_t)d->B * d->H * d->W * d->Cin, d->dx_amax, stream);
}

// 1: the data gradient of this layer (as dispatched for `aux_act`, with the aux tensor present and NO column-sum slab)
// folds max|dx| into d->dx_amax in its own epilogue; 0: by a pass of its own
extern "C" int odin_conv2d_dgrad_keeps_range(const odin_conv_desc* d, int aux_act) {
  const Family f = select_conv2d_dgrad(odin_geom_fwd(d), odin_geom_dgrad(d), aux_act, true, false, false);
  return (traits(f) & FOLDS_DX) ? 1 : 0;
}

// 1: some launch of this layer (forward or weight gradient, as dispatched now for a layer with a bias) is a two-plane
// kernel that READS the range word of the layer input (odin_conv_desc.x_amax) -- a caller uses it to decide whether the
// layer below is asked to keep that word at all (a wrong answer is harmless: a plane kernel without a word carries x
// unscaled, as in round 4)
extern "C" int odin_conv2d_reads_x_range(const odin_conv_desc* d) {
  const odin_geom g = odin_geom_fwd(d);
  return ((traits(select_conv2d_fwd(g, true, d->act)) | traits(select_conv2d_wgrad(g))) & READS_X) ? 1 : 0;
}

// ---- Conv2DTranspose (desc: H,W,Cin = input; OH=H*S, OW=W*S, Cout = output; pads = the SAME pads of the forward conv
// on the OUTPUT size) ----------------------------------------------------------------------------------------------
extern "C" int odin_deconv2d_fwd(const float* x, const float* w, const float* bias, float* y, const odin_conv_desc* d,
                                 void* stream) {
  const odin_geom g = odin_geom_fwd(d);
  return conv_fwd(select_deconv2d_fwd(g, bias != nullptr, d->act), 1, 1, g, x, w, bias, y, d, stream);
}

extern "C" int odin_deconv2d_dgrad(const float* dy, const float* w, const float* aux, int aux_act, float* dx,
                                   float* colsum_slab, int* slab_rows_out, const odin_conv_desc* d, void* stream) {
  const odin_geom g = odin_geom_dgrad(d);
  const Family f = select_deconv2d_dgrad(odin_geom_fwd(d), g, aux_act, aux != nullptr || dx == nullptr,
                                         colsum_slab != nullptr, dx == nullptr);
  return conv_dgrad(f, 0, 0, g, dy, w, aux, aux_act, dx, colsum_slab, slab_rows_out, d, stream);
}

// x = deconv input [B,H,W,Cin], dy = grad wrt deconv pre-activation output [B,OH,OW,Cout]
extern "C" int odin_deconv2d_wgrad(const float* x, const float* dy, float* slab, int* slab_rows_out,
                                   const odin_conv_desc* d, void* stream) {
  const odin_geom g = odin_geom_dgrad(d);
  const Family f = select_deconv2d_wgrad(odin_geom_fwd(d), g);
  if (f == SMALLDECONV)   // (dry run: slab == NULL only reports the rows)
    return odin_smalldeconv_bwd(x, dy, nullptr, nullptr, 0, nullptr, slab, slab_rows_out, d, stream);
  return launch_wgrad(f, g, dy, x, slab, 0, d->dy_amax, d->x_amax, slab_rows_out, stream);
}

extern "C" int odin_deconv2d_bwd(const float* x, const float* dy, const float* w, const float* aux, int aux_act, float* dx,
                                 float* colsum_slab, int* colsum_rows_out, float* wslab, int* wslab_rows_out,
                                 const odin_conv_desc* d, void* stream) {
  const odin_geom l = odin_geom_fwd(d);
  const bool dry = dx == nullptr && wslab == nullptr;
  const Family f = select_deconv2d_bwd(l, odin_geom_dgrad(d), aux_act, aux != nullptr, dx != nullptr && wslab != nullptr,
                                       dry, colsum_slab != nullptr);
  if (f == SMALLDECONV) {
    if (colsum_rows_out) *colsum_rows_out = 0;
    return odin_smalldeconv_bwd(x, dy, w, aux, aux_act, dx, wslab, wslab_rows_out, d, stream);
  }
  if (f == BWD_PLANES || f == BWD_BLK) {
    const int rows = f == BWD_PLANES ? odin_bwd_planes_rows(l) : odin_bwd_blk_rows(l);
    if (colsum_rows_out) *colsum_rows_out = rows;
    if (wslab_rows_out) *wslab_rows_out = rows;
    if (dry) return 0;
    if (f == BWD_PLANES)
      return odin_bwd_planes_launch(x, dy, w, aux, dx, colsum_slab, wslab, d->B, d->H, d->W, d->Cin, d->Cout, d->dy_amax,
                                    d->x_amax, d->dx_amax, stream);
    return odin_bwd_blk_launch(x, dy, w, aux, aux_act, dx, colsum_slab, wslab, d->B, d->H, d->W, d->Cin, d->Cout,
                               d->dy_amax, d->x_amax, d->dx_amax, stream);
  }
  odin_igemm_pair_begin();
  int rc = odin_deconv2d_wgrad(x, dy, wslab, wslab_rows_out, d, stream);
  if (rc == 0) rc = odin_deconv2d_dgrad(dy, w, aux, aux_act, dx, colsum_slab, colsum_rows_out, d, stream);
  return pair_end(rc);
}

extern "C" int odin_deconv2d_dgrad_keeps_range(const odin_conv_desc* d, int aux_act) {
  const Family f = select_deconv2d_dgrad(odin_geom_fwd(d), odin_geom_dgrad(d), aux_act, true, false, false);
  return (traits(f) & FOLDS_DX) ? 1 : 0;
}
extern "C" int odin_deconv2d_reads_x_range(const odin_conv_desc* d) {
  const odin_geom l = odin_geom_fwd(d);
  return ((traits(select_deconv2d_fwd(l, true, d->act)) | traits(select_deconv2d_wgrad(l, odin_geom_dgrad(d)))) & READS_X)
             ? 1 : 0;
}

// ---- fused decoder tail: (Conv2DTranspose | Conv2D)(act) -> Conv2D 1x1 linear (C1<=4 maps)
// -> Independent(Bernoulli).log_prob(target), forward + backward in one launch ----------
extern "C" int odin_bernoulli_tail_fwd_bwd(int is_deconv, const float* x, const float* w, const float* bias, const float* w1,
                                           const float* b1, const float* target, float* logits, float* g_out,
                                           float* llk_part, int* n_part_out, float* tail_slab, int* slab_rows_out,
                                           const float* scale, const odin_conv_desc* d, int C1, void* stream) {
  const odin_geom g = odin_geom_fwd(d);
  const Family f = select_bernoulli_tail(is_deconv, g, d->act, C1);
  const odin_tail_args tail = {w1, b1, target, scale, logits, llk_part, tail_slab, C1};
  int rc;
  if (f == TCONV_PLANES)
    rc = odin_tconv_planes_launch(x, w, bias, nullptr, g_out, nullptr, slab_rows_out, w1, b1, target, logits, llk_part,
                                  n_part_out, tail_slab, scale, C1, d->B, d->H, d->W, d->Cin, d->Cout, 3, d->x_amax,
                                  d->dy_amax, stream);
  else if (f == TCONV_RING)
    rc = odin_tconv_ring_launch(x, w, bias, nullptr, g_out, nullptr, slab_rows_out, w1, b1, target, logits, llk_part,
                                n_part_out, tail_slab, scale, C1, d->B, d->H, d->W, d->Cout, 3, stream);
  else
    rc = odin_gather_generic(is_deconv, is_deconv ? 1 : 0, g, x, w, bias, d->act, nullptr, 0, g_out, nullptr,
                             -ODIN_MAX_COLSUM_BLOCKS, slab_rows_out, &tail, n_part_out, stream);
  // (the range contract: a word handed in as d->dy_amax bounds g_out on return)
  return keep_range(rc, f, FOLDS_Y, g_out, (size_t)d->B * d->OH * d->OW * d->Cout, d->dy_amax, stream);
}
// the tail with the Conv2DTranspose below it in the same launch: only where BOTH layers are the plane kernels' (the
// selectors' answer, so that every switch that turns those off turns the chain off too)
extern "C" int odin_decoder_tail_chain(const float* x, const float* w3, const float* b3, float* y3, const odin_conv_desc* d3,
                                       const float* w4, const float* b4, const float* w1, const float* b1,
                                       const float* target, float* logits, float* g_out, float* llk_part, int* n_part_out,
                                       float* tail_slab, int* slab_rows_out, int* same_partition_out, const float* scale,
                                       const odin_conv_desc* d4, int C1, void* stream) {
  const odin_geom g3 = odin_geom_fwd(d3), g4 = odin_geom_fwd(d4);
  if (select_deconv2d_fwd(g3, true, d3->act) != TCONV_PLANES || select_bernoulli_tail(1, g4, d4->act, C1) != TCONV_PLANES ||
      !odin_tconv_chain2_applicable(g3, g4, C1))
    return odin_fail(-2, "decoder_tail_chain: shapes outside the chain");
  return odin_tconv_chain2_launch(x, w3, b3, y3, w4, b4, w1, b1, target, logits, g_out, llk_part, n_part_out, tail_slab,
                                  slab_rows_out, same_partition_out, scale, C1, d3->B, d3->x_amax, d3->y_amax, d4->dy_amax,
                                  stream);
}
// 1: the fused tail folds max|g_out| into d->dy_amax itself
extern "C" int odin_bernoulli_tail_keeps_range(int is_deconv, const odin_conv_desc* d, int C1) {
  return (traits(select_bernoulli_tail(is_deconv, odin_geom_fwd(d), d->act, C1)) & FOLDS_Y) ? 1 : 0;
}

// ---- Dense: y[B,N] = act(x[B,K] @ w[K,N] + b) ------------------------------------------------------------------------
extern "C" int odin_dense_fwd(const float* x, const float* w, const float* bias, float* y, int B, int K, int N, int act,
                              void* stream) {
  return odin_dense_fwd_ranged(x, w, bias, y, B, K, N, act, nullptr, nullptr, stream);
}

// the same with the activation range words (include/odin_hip.h: the range contract): x_amax is read by the two-plane
// GEMM, y_amax is valid on return whatever family ran
extern "C" int odin_dense_fwd_ranged(const float* x, const float* w, const float* bias, float* y, int B, int K, int N,
                                     int act, const uint32_t* x_amax, uint32_t* y_amax, void* stream) {
  const Family f = select_dense_fwd(B, K, N, aligned16(x, w, y, bias));
  int rc;
  switch (f) {
    case TINY_DENSE: rc = odin_tiny_dense_fwd(x, w, bias, y, B, K, N, act, stream); break;
    case THIN_DENSE: rc = odin_thin_dense_fwd(x, w, bias, y, B, K, N, act, y_amax, stream); break;
    case DENSE_H: rc = odin_dense_h_fwd(x, w, bias, y, B, K, N, act, x_amax, y_amax, stream); break;
    case DENSE_GEMM: rc = odin_dense_gemm_fwd(x, w, bias, y, B, K, N, act, stream); break;
    default:   // the implicit GEMM or the generic gather
      rc = launch_gather(f, 0, 0, odin_geom_dense(B, K, N), x, w, bias, nullptr, 0, y, nullptr, nullptr, 1, act, nullptr,
                         y_amax, stream);
  }
  return keep_range(rc, f, FOLDS_Y, y, (size_t)B * N, y_amax, stream);
}

// dx[B,K] = (dy[B,N] @ w[K,N]^T) * act'(aux), with the range words of dy (read by the plane GEMM) and dx (valid on
// return, as the convolutions')
static int dense_dgrad(const float* dy, const float* w, const float* aux, int aux_act, float* dx, float* colsum_slab,
                       int* slab_rows_out, int B, int K, int N, const uint32_t* dy_amax, uint32_t* dx_amax,
                       void* stream) {
  const Family f = select_dense_dgrad(B, K, N, colsum_slab != nullptr, aligned16(dy, w, dx, aux));
  if (f != TINY_DENSE && f != GENERIC) {   // (no column sums from these families)
    if (slab_rows_out) *slab_rows_out = 0;
    if (dx == nullptr) return 0;  // dry run
  }
  int rc;
  switch (f) {
    case TINY_DENSE:
      rc = odin_tiny_dense_dgrad(dy, w, aux, aux_act, dx, colsum_slab, slab_rows_out, B, K, N, stream);
      break;
    case THIN_DENSE: rc = odin_thin_dense_dgrad(dy, w, aux, aux_act, dx, B, K, N, dx_amax, stream); break;
    case DENSE_H: rc = odin_dense_h_dgrad(dy, w, aux, aux_act, dx, B, K, N, dy_amax, dx_amax, stream); break;
    case DENSE_GEMM: rc = odin_dense_gemm_dgrad(dy, w, aux, aux_act, dx, B, K, N, dx_amax, stream); break;
    default:   // the implicit GEMM as a transposed gather; the generic kernel as a strided one over the same weight layout
      rc = launch_gather(f, f == IGEMM, 1, odin_geom_dense(B, N, K), dy, w, nullptr, aux, aux_act, dx, colsum_slab,
                         slab_rows_out, 2, 0, nullptr, dx_amax, stream);
  }
  return keep_range(rc, f, FOLDS_DX, dx, (size_t)B * K, dx_amax, stream);
}

extern "C" int odin_dense_dgrad(const float* dy, const float* w, const float* aux, int aux_act, float* dx,
                                float* colsum_slab, int* slab_rows_out, int B, int K, int N, void* stream) {
  // (no range words through this entry: a plane GEMM bounds dy itself)
  return dense_dgrad(dy, w, aux, aux_act, dx, colsum_slab, slab_rows_out, B, K, N, nullptr, nullptr, stream);
}

extern "C" int odin_dense_wgrad(const float* x, const float* dy, float* slab, int* slab_rows_out, int B, int K, int N,
                                void* stream) {
  const Family f = select_dense_wgrad(B, K, N, slab == nullptr || aligned16(x, dy, slab, nullptr));
  if (f == DENSE_H || f == THIN_DENSE || f == DENSE_GEMM) {
    if (slab_rows_out) *slab_rows_out = f == THIN_DENSE ? odin_thin_dense_wgrad_rows(B, K, N) : 1;
    if (slab == nullptr) return 0;  // dry run
    if (f == DENSE_H) return odin_dense_h_wgrad(x, dy, slab, B, K, N, nullptr, nullptr, stream);
    if (f == THIN_DENSE) return odin_thin_dense_wgrad(x, dy, slab, B, K, N, stream);
    return odin_dense_gemm_wgrad(x, dy, slab, B, K, N, stream);
  }
  return launch_wgrad(f, odin_geom_dense(B, K, N), x, dy, slab, 1, nullptr, nullptr, slab_rows_out, stream);
}

// want_wgrad / want_dgrad: either half may be left out (FactorVAE's TC term back-propagates through the discriminator
// without touching its weights).  dy_amax / dx_amax: the range words of dy (read) and dx (written), both optional.
extern "C" int odin_dense_bwd(const float* x, const float* dy, const float* w, const float* aux, int aux_act, float* dx,
                              float* colsum_slab, int* colsum_rows_out, float* wslab, int* wslab_rows_out, int B, int K,
                              int N, int want_wgrad, int want_dgrad, const uint32_t* dy_amax, uint32_t* dx_amax, void* stream) {
  return odin_dense_bwd_ranged(x, dy, w, aux, aux_act, dx, colsum_slab, colsum_rows_out, wslab, wslab_rows_out, B, K, N,
                               want_wgrad, want_dgrad, dy_amax, dx_amax, nullptr, stream);
}

// + x_amax: the range word of the activation x (the weight gradient's other operand on the two-plane GEMM)
extern "C" int odin_dense_bwd_ranged(const float* x, const float* dy, const float* w, const float* aux, int aux_act,
                                     float* dx, float* colsum_slab, int* colsum_rows_out, float* wslab, int* wslab_rows_out,
                                     int B, int K, int N, int want_wgrad, int want_dgrad, const uint32_t* dy_amax,
                                     uint32_t* dx_amax, const uint32_t* x_amax, void* stream) {
  if (select_dense_bwd(B, K, N, colsum_slab != nullptr) == DENSE_H) {
    int rc = 0;
    // (a dy without a word is bounded ONCE for both halves)
    if (dy_amax == nullptr && ((want_wgrad && wslab != nullptr) || (want_dgrad && dx != nullptr))) {
      dy_amax = odin_range_word_of(dy, (size_t)B * N, nullptr, stream);
      if (dy_amax == nullptr) return odin_fail(-3, "dense_bwd: no range word for dy");
    }
    if (want_wgrad && want_dgrad && wslab != nullptr && dx != nullptr) {
      // both halves: ONE launch (dense_h.hip: dense_h_pair_kernel), bit-identical to the two
      if (wslab_rows_out) *wslab_rows_out = 1;
      if (colsum_rows_out) *colsum_rows_out = 0;
      return odin_dense_h_bwd_pair(x, dy, w, aux, aux_act, dx, wslab, B, K, N, dy_amax, dx_amax, x_amax, stream);
    }
    if (want_wgrad) {
      if (wslab_rows_out) *wslab_rows_out = 1;
      if (wslab != nullptr) rc = odin_dense_h_wgrad(x, dy, wslab, B, K, N, dy_amax, x_amax, stream);
    }
    if (rc == 0 && want_dgrad) {
      if (colsum_rows_out) *colsum_rows_out = 0;
      if (dx != nullptr) rc = odin_dense_h_dgrad(dy, w, aux, aux_act, dx, B, K, N, dy_amax, dx_amax, stream);
    }
    return rc;
  }
  odin_igemm_pair_begin();
  int rc = 0;
  if (want_wgrad) rc = odin_dense_wgrad(x, dy, wslab, wslab_rows_out, B, K, N, stream);
  if (rc == 0 && want_dgrad)
    rc = dense_dgrad(dy, w, aux, aux_act, dx, colsum_slab, colsum_rows_out, B, K, N, dy_amax, dx_amax, stream);
  return pair_end(rc);
}

// 1: the data gradient of this Dense layer (without a column-sum slab, 16-byte aligned tensors) folds max|dx| into
// dx_amax itself
extern "C" int odin_dense_dgrad_keeps_range(int B, int K, int N) {
  return (traits(select_dense_dgrad(B, K, N, false, true)) & FOLDS_DX) ? 1 : 0;
}
extern "C" int odin_dense_reads_x_range(int B, int K, int N) {
  return (traits(select_dense_fwd(B, K, N, true)) & READS_X) ? 1 : 0;
}
