// mv_conv.h -- host side of the convolutions: the general-cin 3x3 with K slices across workgroups (conv3x3_gen.hip), and nn.Conv2d
// of any geometry (conv_igemm.hip: launch_conv2d; its columns form is deform.hip's launch_conv2d_columns)
#pragma once
#include "mv_common.h"

namespace mv {

// slices == 1: one ascending (channel, ky, kx) chain per output; otherwise `slices` chains over `slice_channels` input channels
// each (the last may be shorter), added in ascending slice order, then bias, then ReLU
void conv3x3_gen_plan(int64_t n, int cin, int h, int wdt, int cout, int* slices, int* slice_channels);
int64_t conv3x3_gen_workspace_bytes(int64_t n, int cin, int h, int wdt, int cout);
// workspace == nullptr: the single chain (== launch_conv3x3_gen)
int launch_conv3x3_gen_ws(const float* x, const float* w, const float* b, float* y, int64_t n, int cin, int h, int wdt, int cout,
                          int relu, hipStream_t s, void* workspace, int64_t workspace_bytes);

// A convolution's geometry on the host (never a kernel argument).  The caller writes the first 13 members, conv2d_geometry()
// (abi.hip) validates them and sets oh / ow; the launchers below take it checked, with cin and cout multiples of groups.
struct Conv2dGeom {
  int cin, h, w, cout, kh, kw, sh, sw, ph, pw, dh, dw, groups;
  int oh = 0, ow = 0;
};

// Which form a convolution runs in -- also what mv_conv2d_needs_workspace() / mv_deform_conv2d_needs_workspace() answer
enum ConvForm {
  kFormDirect = 0,   // no columns in HBM (implicit GEMM; deformable: the fused kernel); the workspace is not used
  kFormColumns = 1,  // columns into the workspace + the pointwise GEMM: the only form that covers this geometry
  kFormEither = 2,   // a launch too small to fill the chip with the direct form's tiles: columns if the caller brought a workspace
};
inline int64_t columns_bytes_per_image(const Conv2dGeom& g) { return (int64_t)sizeof(float) * g.cin * g.kh * g.kw * g.oh * g.ow; }
// the form's answer together with the workspace that was passed
inline bool takes_columns(ConvForm form, const Conv2dGeom& g, const void* workspace, int64_t workspace_bytes) {
  return form == kFormColumns || (form == kFormEither && workspace != nullptr && workspace_bytes >= columns_bytes_per_image(g));
}

// the whole tensor's epilogue at weight group `group`'s first channel; the residual (shaped like y) from image b0 on
inline Epilogue group_epilogue(Epilogue e, const Conv2dGeom& g, int group, int64_t b0) {
  const size_t c0 = (size_t)group * (g.cout / g.groups);
  if (e.bias) e.bias += c0;
  if (e.alpha) e.alpha += c0;
  if (e.beta) e.beta += c0;
  if (e.res) e.res += ((size_t)b0 * g.cout + c0) * ((int64_t)g.oh * g.ow);
  return e;
}

// conv_igemm.hip -- nn.Conv2d of any geometry: launch_conv2d picks the form and runs the weight groups (`whole`: the whole tensor's
// epilogue, whole.res shaped like y); launch_conv2d_implicit is one group of the implicit form, x, w, y and e at its first channel
ConvForm conv2d_form(int64_t n, const Conv2dGeom& g);
int launch_conv2d(const float* x, const float* weight, float* y, int64_t n, const Conv2dGeom& g, const Epilogue& whole, void* workspace,
                  int64_t workspace_bytes, hipStream_t s);
int launch_conv2d_implicit(const float* x, const float* w, float* y, int64_t n, const Conv2dGeom& g, const Epilogue& e, hipStream_t s);

// deform.hip -- the columns form of both convolutions.  offset == nullptr: plain im2col (mask and offset_groups unused); else
// deformable, mask == nullptr: no modulation.  A workspace below one image's columns is an error.
int launch_conv2d_columns(const float* x, const float* weight, const float* offset, const float* mask, float* y, int64_t n,
                          const Conv2dGeom& g, int offset_groups, const Epilogue& whole, void* workspace, int64_t workspace_bytes,
                          hipStream_t s);

}  // namespace mv
