// The discriminators' weights as the handle holds them: shared by the passes (discriminator.hip) and the optimizer step (disc_optim.hip).
#pragma once
#include "model_common.h"
#include "models.h"

namespace rvc {

struct DiscLayer {
  int Ci = 0, Co = 0, k = 0, stride = 1, pad = 0, groups = 1, CoPx = 0;
  DevVec w, b;                       // folded fp32 weights [Co][Ci / groups][k] (the VALU layers) and bias
  DevBuf<uint16_t> wx;               // bf16x3 image (the GEMM layers)
  DevBuf<uint16_t> wxb[3];           // the GEMM layers' data gradient: one transposed image per phase of the input row (stride of them), rows Ci padded to CiPx
  int CiPx = 0;
  DevVec pv, pg;                     // weight_v [Co][Ci / groups][k] and weight_g [Co] as loaded: only with disc_keep_parameters (the weight-norm chain of weight_grad).
                                     // A plain-weight net kept for training holds the fp32 master copy of a GEMM layer's weight in pv (its VALU layers' master is w)
  int gi_w = -1, gi_g = -1, gi_b = -1;   // this layer's entries of the parameter list: weight_v (or the plain weight), weight_g (-1: plain weight), bias
};
struct DiscParam { std::string name; std::vector<long long> shape; };
struct DiscNet { int period = 0; std::vector<DiscLayer> L; };   // period 0: DiscriminatorS; L.back() is conv_post
struct DiscWeights { std::vector<DiscNet> nets; };
struct DiscOptimTables;              // disc_optim.hip: the device tables of the optimizer step, made by the first step of a handle
struct Disc : DiscWeights {
  Ctx* ctx = nullptr;
  int version = 2;
  TensorStore ts;
  bool ready = false;
  bool keep = false;                 // disc_keep_parameters: finalize keeps weight_v / weight_g on the device and weight_grad is allowed
  bool kept = false;                 // what the finalized net was loaded with
  std::vector<DiscParam> params;     // the parameter tensors in the reference module's state-dict order (per layer: bias, weight_g, weight_v; or weight, bias)
  std::shared_ptr<DiscOptimTables> optim;   // null until the first optimizer step / set_parameters; dropped by finalize
};

inline bool disc_layer_is_gemm(const DiscLayer& l) { return l.groups == 1 && l.Ci % 16 == 0 && l.Co > 1; }

}  // namespace rvc
