// Fused backward of one conv / convT layer: dispatch.
//
// The separate kernels of conv_mfma.hip read the upstream gradient twice: the backward-data kernel stages
// dU = relu'(y) * BatchNorm-backward(g) to convolve it with the flipped weights, and the weight-gradient kernel
// stages the same dU again to correlate it with the layer input.  A fused kernel stages, per tile,
//   * the dU window (with the halo the data gradient needs; prologue PRO_BWD or PRO_ID applied on the way in), and
//   * the layer-input window x_n = BatchNorm(x) (with the halo the weight gradient needs, zero padded),
// and runs both implicit GEMMs off those two LDS tiles:
//   dx[p][ci]        = sum_{tap,co} dU[p (+) tap][co] * Gb[tap][co][ci]      (+ sum dx, sum dx*xhat for BatchNorm l)
//   dG[tap][ci][co] += sum_{p in tile interior} x_n[p (+) tap][ci] * dU[p][co],   db[co] += sum_p dU[p][co]
// so g, y and x are fetched from HBM once per layer instead of twice (reference: autograd's conv backward,
// ava/models/vae.py:347-353 loss.backward()).  Tiles are indexed in the LOW-resolution space of the layer
// (S1: both tensors; stride-2 conv: the dU side; stride-2 convT: the x side).
//
// The kernels are the thin (1 <-> 8-channel) VALU kernels of conv_thin.hip and the bf16 limb-MFMA kernels of
// conv_fused_limb.hip, whose tiles divide every supported image size (W in {128, 256}, H a multiple of 128:
// low-resolution sides >= 16 against tiles of at most 32 x 8).  A shape neither serves reports "no fused kernel"
// (grid 0); the model driver treats that as an error, it has no second path.
#include "conv_fused.h"

// number of workgroups (= partial rows of both outputs) of the fused kernel, 0 when the shape has none
int ava_conv_fused_grid_for(int B, int Hi, int Wi, int Cin, int Cout, int mode) {
  const int thin = ava_thin_fused_grid(B, Hi, Wi, Cin, Cout, mode);
  if (thin > 0) return thin;
  int tw, th;
  const int hl = mode == MODE_DOWN ? Hi / 2 : Hi, wl = mode == MODE_DOWN ? Wi / 2 : Wi;
  const int lcap = ava_conv_fused_limb_cap(Cin, Cout, mode, &tw, &th);   // the limb kernel's own tile and resident-wave size
  if (lcap > 0 && hl % th == 0 && wl % tw == 0) {
    const int nt = B * (hl / th) * (wl / tw);
    return nt < ava_scale_grid(lcap) ? nt : ava_scale_grid(lcap);
  }
  return 0;
}

int ava_conv3x3_bwd_fused_launch(const FusedArgs& a, int Cin, int Cout, int mode, int dy_pro, hipStream_t st) {
  const int grid = ava_conv_fused_grid_for(a.B, a.Hi, a.Wi, Cin, Cout, mode);
  if (grid <= 0) return AVA_EINVAL;
  if (Cin == 1 || Cout == 1) return ava_thin_bwd_fused_launch(a, grid, Cin, dy_pro, st);
  if (a.dx == nullptr) return AVA_EINVAL;
  if (!ava_conv_fused_limb_has(Cin, Cout, mode)) return AVA_EINVAL;
  return ava_conv3x3_bwd_fused_limb_launch(a, grid, Cin, Cout, mode, dy_pro, st);   // AVA_EINVAL: the image does not divide into its tiles
}

extern "C" int ava_conv_fused_grid(int B, int Hi, int Wi, int Cin, int Cout, int mode) {
  return ava_conv_fused_grid_for(B, Hi, Wi, Cin, Cout, mode);
}

extern "C" int ava_conv3x3_bwd_fused(const float* x, const float* xa, const float* xb, const float* dy, const float* dy2,
                                     const float* da, const float* db, const float* dc, const float* Gb, float* dx,
                                     const float* mean, const float* invstd, float* bn_partials, float* wg_partials,
                                     int B, int Hi, int Wi, int Cin, int Cout, int mode, int dy_pro, ava_stream_t s) {
  if (x == nullptr || xa == nullptr || xb == nullptr || dy == nullptr || Gb == nullptr || (dx == nullptr && Cin != 1) ||
      mean == nullptr || invstd == nullptr || bn_partials == nullptr || wg_partials == nullptr || B < 1)
    return AVA_EINVAL;
  if (dy_pro == PRO_BWD && (dy2 == nullptr || da == nullptr || db == nullptr || dc == nullptr)) return AVA_EINVAL;
  FusedArgs a = {};
  a.x = x; a.xa = xa; a.xb = xb; a.dy = dy; a.dy2 = dy2; a.da = da; a.db = db; a.dc = dc; a.Gb = Gb; a.dx = dx;
  a.mean = mean; a.invstd = invstd; a.bn_partials = bn_partials; a.wg_partials = wg_partials;
  a.act_bf16 = 0;
  a.acc_out = nullptr;
  a.fin = BnFin{};
  a.B = B; a.Hi = Hi; a.Wi = Wi;
  a.Ho = mode == MODE_S1 ? Hi : (mode == MODE_DOWN ? Hi / 2 : Hi * 2);
  a.Wo = mode == MODE_S1 ? Wi : (mode == MODE_DOWN ? Wi / 2 : Wi * 2);
  a.tiles_y = a.tiles_x = a.ntiles = 0;
  return ava_conv3x3_bwd_fused_launch(a, Cin, Cout, mode, dy_pro, to_stream(s));
}
