// mv_deform.h -- deform_conv2d's two forms: deform_fused.hip (no columns in HBM) and deform.hip (columns workspace + GEMM)
#pragma once
#include "mv_conv.h"

namespace mv {

// workgroups the fused launch would have (0: its tiles do not fit this geometry)
int64_t deform_fused_workgroups(int64_t n, const Conv2dGeom& g, int offset_groups);
// mask == nullptr: no modulation; bias == nullptr: none
int launch_deform_fused(const float* x, const float* weight, const float* offset, const float* mask, const float* bias, float* y,
                        int64_t n, const Conv2dGeom& g, int offset_groups, hipStream_t s);

// deform.hip: the fused kernel or the columns form (launch_conv2d_columns), as deform_conv2d_form() says and the workspace allows
ConvForm deform_conv2d_form(int64_t n, const Conv2dGeom& g, int offset_groups);
int launch_deform_conv2d(const float* x, const float* weight, const float* offset, const float* mask, const float* bias, float* y,
                         int64_t n, const Conv2dGeom& g, int offset_groups, void* workspace, int64_t workspace_bytes, hipStream_t s);

}  // namespace mv
