"""mi355vision -- the MI355X (gfx950) implementation of CPU-Vision's image-filtering hot path.

Python host layer (the reference is Python) over the C ABI in include/mi355vision.h:
  functional      the one namespace of the functional surface: the module-level switches, and re-exports of
  _filters        gaussian_blur / adjust_sharpness (+ _image/_video kernels, *_frames), box / separable / Sobel
  _layers         conv+ReLU, pools, linear, conv_norm_act, dwconv_pointwise, inverted_residual (what nn, mobilenet and ssdlite run on)
  _misc           resize / center_crop / to_dtype / normalize (+ kernels), to_float_normalize
  _detection      rpn_topk / rpn_decode / box_decode (what rpn runs on), roi_detections (what roi_heads runs on), retinanet_topk /
                  retinanet_decode (what retinanet runs on), fcos_topk / fcos_decode (what fcos runs on)
  _norm           group_norm_act: GroupNorm (+ ReLU), float64 statistics, two launches; l2_normalize_scale: weight * F.normalize over the
                  channels (SSD's conv4_3), float64 sum of squares, one launch
  _crop, _mix     pad / crop / flip / erase / resized_crop; MixUp / CutMix on a batch
  functional_v1   the v1 tensor backend's gaussian_blur / adjust_sharpness, resize / center_crop
  mobilenet       Conv2dNormActivation with a folded norm, InvertedResidual, MobileNetV2, SqueezeExcitation
  mobilenetv3     InvertedResidualConfig, InvertedResidual (5x5 depthwise; the squeeze-excitation gate folded into the projection's loads),
                  MobileNetV3, mobilenet_v3_large / mobilenet_v3_small (dilated=True: a segmentation backbone, its depthwise 5x5 convs
                  at dilation 2 one launch each); _se: global_avg_pool, linear_act, se_scale (float64 sums)
  resnet          BasicBlock / Bottleneck / ResNet, resnet18 ... resnet152, wide_resnet50_2 / 101_2: one launch per conv + norm (+ add) + ReLU
  fpn             FeaturePyramidNetwork, LastLevelMaxPool, LastLevelP6P7: lateral 1x1 conv + nearest upsample + add in one launch
  backbone_utils  IntermediateLayerGetter, BackboneWithFPN, resnet_fpn_backbone
  anchor_utils    AnchorGenerator, DefaultBoxGenerator (SSD's default boxes); image_list: ImageList
  rpn             BoxCoder (decode), RPNHead (cls_logits + bbox_pred as one pointwise launch), RegionProposalNetwork: top-k on the
                  head's NCHW maps, then anchors + decode + clip + sigmoid of the selected candidates only, then batched_nms
  roi_heads       RoIHeads: pooler -> box head -> predictor -> softmax + decode + clip + filters of every (roi, class) in one launch,
                  then batched_nms per class
  faster_rcnn     FasterRCNN, TwoMLPHead, FastRCNNPredictor (cls_score + bbox_pred as one linear launch), fasterrcnn_resnet50_fpn;
                  generalized_rcnn: GeneralizedRCNN; transform: GeneralizedRCNNTransform (normalize + resize + batch as one launch)
  mask_rcnn       MaskRCNN, MaskRCNNHeads, MaskRCNNPredictor (ConvTranspose2d(2, 2) + ReLU as one pixel-shuffling pointwise launch),
                  maskrcnn_resnet50_fpn; _mask: mask_probs (gather + sigmoid) and paste_masks_in_image (one launch per image)
  keypoint_rcnn   KeypointRCNN, KeypointRCNNHeads, KeypointRCNNPredictor (ConvTranspose2d(4, stride 2, padding 1) as one implicit-GEMM
                  launch with a transposed store, then the x2 bilinear interpolate), keypointrcnn_resnet50_fpn; _keypoint:
                  heatmaps_to_keypoints (bicubic resize + argmax of every (roi, keypoint) in one launch, nothing materialised)
  retinanet       RetinaNetClassificationHead / RetinaNetRegressionHead / RetinaNetHead (the towers' first convs as one launch),
                  RetinaNet: threshold + top-k over every (anchor, class) of the heads' NCHW maps, many workgroups per (image,
                  level), then decode + clip + sigmoid of the selected candidates only, then batched_nms; retinanet_resnet50_fpn
  fcos            FCOSClassificationHead / FCOSRegressionHead / FCOSHead (towers of conv, then GroupNorm + ReLU: _norm.group_norm_act),
                  FCOS: threshold + top-k on sqrt(sigmoid(cls) * sigmoid(centerness)), BoxLinearCoder's linear decode of the selected
                  candidates only, then batched_nms; fcos_resnet50_fpn
  ssd             SSDFeatureExtractorVGG (VGG16 with the ceil-mode third pool, conv4_3 rescaled by _norm.l2_normalize_scale, the dilated
                  fc6), SSDHead (one conv launch per level and head), SSD: softmax into a class-major matrix, per-class threshold +
                  top-k on its rows, default boxes + decode of the selected candidates only, then batched_nms; ssd300_vgg16
  ssdlite         SSDLiteFeatureExtractorMobileNet (MobileNetV3-Large split at the C4 expansion, four extra blocks), SSDLiteHead: every
                  depthwise-separable block (depthwise 3x3 + norm + ReLU6 -> 1x1 conv) one launch, the depthwise stage computed in the
                  pointwise kernel's loads (_layers.dwconv_pointwise); ssdlite320_mobilenet_v3_large on ssd.SSD
  segmentation    FCN / FCNHead, DeepLabV3 / DeepLabHead / ASPP / ASPPConv / ASPPPooling on the dilated ResNets (a 1x1 conv + norm + ReLU one
                  launch; the heads' 3x3 convs the implicit GEMM at padding = dilation = rate, one launch per 128 input channels), fcn_resnet50 / 101, deeplabv3_resnet50 / 101;
                  LRASPP / LRASPPHead (five launches: the gate product and the upsample in the high classifier's loads, the low
                  classifier as its residual), lraspp_mobilenet_v3_large, deeplabv3_mobilenet_v3_large on the dilated MobileNetV3;
                  model.labels(x): _segment.interpolate_argmax, the final resize + argmax as one launch that writes only the labels
  ops             deform_conv2d / DeformConv2d, nms / batched_nms, roi_align / RoIAlign, roi_pool / RoIPool, ps_roi_pool / PSRoIPool,
                  ps_roi_align / PSRoIAlign (+ registration behind torch.ops.torchvision.*); box_iou / generalized_box_iou /
                  distance_box_iou, masks_to_boxes, MultiScaleRoIAlign, box_area / box_convert / clip_boxes_to_image /
                  remove_small_boxes
  graphs          HIP-graph capture of a whole forward (batch-1 latency)
  presets         ImageClassification (resize -> center_crop -> float -> normalize in one call)
  transforms      GaussianBlur, RandomAdjustSharpness, GaussianBlurV1, the geometric and colour v2 transforms
  nn              Conv3x3ReLU, VGG / AlexNet (re-exports mobilenet.Conv2dNormActivation: one class under that name)
  sharding        frame-block partitioning over the GPUs of a node (no data-path collective)
  register_kernel the reference's kernel-registry plugin surface

The directory is named `cpu-vision_amd`; import it as `cpu_vision_amd` (alias package at the repo root).
"""
from . import (anchor_utils, backbone_utils, faster_rcnn, fcos, fpn, functional, functional_v1, generalized_rcnn, graphs, image_list,  # noqa: F401
               keypoint_rcnn, mask_rcnn, mobilenet, mobilenetv3, nn, ops, presets, resnet, retinanet, roi_heads, rpn, segmentation, sharding, ssd,
               ssdlite, transform, transforms, tv_tensors)
from ._lib import LIB_PATH, Mi355VisionError, load as load_library  # noqa: F401
from ._registry import register_kernel  # noqa: F401
from .backbone_utils import BackboneWithFPN, IntermediateLayerGetter, resnet_fpn_backbone  # noqa: F401
from .fpn import ExtraFPNBlock, FeaturePyramidNetwork, LastLevelMaxPool, LastLevelP6P7  # noqa: F401
from .anchor_utils import AnchorGenerator, DefaultBoxGenerator  # noqa: F401
from .image_list import ImageList  # noqa: F401
from .rpn import BoxCoder, RegionProposalNetwork, RPNHead  # noqa: F401
from .roi_heads import RoIHeads  # noqa: F401
from .transform import GeneralizedRCNNTransform  # noqa: F401
from .generalized_rcnn import GeneralizedRCNN  # noqa: F401
from .faster_rcnn import FasterRCNN, FastRCNNPredictor, TwoMLPHead, fasterrcnn_resnet50_fpn  # noqa: F401
from .mask_rcnn import MaskRCNN, MaskRCNNHeads, MaskRCNNPredictor, maskrcnn_resnet50_fpn  # noqa: F401
from .keypoint_rcnn import KeypointRCNN, KeypointRCNNHeads, KeypointRCNNPredictor, keypointrcnn_resnet50_fpn  # noqa: F401
from .retinanet import (RetinaNet, RetinaNetClassificationHead, RetinaNetHead, RetinaNetRegressionHead,  # noqa: F401
                        retinanet_resnet50_fpn)
from .fcos import FCOS, FCOSClassificationHead, FCOSHead, FCOSRegressionHead, fcos_resnet50_fpn  # noqa: F401
from .ssd import (SSD, SSDClassificationHead, SSDFeatureExtractorVGG, SSDHead, SSDRegressionHead, SSDScoringHead,  # noqa: F401
                  ssd300_vgg16)
from .ssdlite import (SSDLiteClassificationHead, SSDLiteFeatureExtractorMobileNet, SSDLiteHead, SSDLiteRegressionHead,  # noqa: F401
                      ssdlite320_mobilenet_v3_large)
from .mobilenet import refresh_parameters  # noqa: F401
from .mobilenetv3 import MobileNetV3, mobilenet_v3_large, mobilenet_v3_small  # noqa: F401
from .segmentation import (ASPP, FCN, LRASPP, ASPPConv, ASPPPooling, DeepLabHead, DeepLabV3, FCNHead, LRASPPHead,  # noqa: F401
                           deeplabv3_mobilenet_v3_large, deeplabv3_resnet50, deeplabv3_resnet101, fcn_resnet50, fcn_resnet101,
                           lraspp_mobilenet_v3_large)
from .ops import (MultiScaleRoIAlign, box_area, box_convert, box_iou, clip_boxes_to_image, distance_box_iou,  # noqa: F401
                  generalized_box_iou, masks_to_boxes, remove_small_boxes)
from .functional import (adjust_sharpness, adjust_sharpness_image, box_filter, conv2d_bias_relu,  # noqa: F401
                         depthwise_conv2d, gaussian_blur, gaussian_blur_image, gaussian_sobel,
                         separable_gaussian_blur, sobel)

__version__ = "0.1.0"
