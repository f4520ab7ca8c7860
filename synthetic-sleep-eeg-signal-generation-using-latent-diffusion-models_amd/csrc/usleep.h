// U-Sleep executor state shared by the forward (usleep.hip) and the training path (usleep_train.hip).
#pragma once
#include <string>
#include <vector>

#include "net.h"

namespace {
constexpr int UT = 256;            // 4 waves: wave = channel group (4 output channels), lane = one of 64 flattened (sample, position) rows
constexpr int UROWS = 64;
constexpr int UCO = 16;            // output channels per block
constexpr int UCI = 32;            // input channels per LDS weight stage
constexpr int UKMAX = 16;

struct ConvSrc {
  const float* a; int Ca, La, ups;     // channels [0, Ca): a[b][ci][ups ? p / 2 : p], p < L
  const float* b2; int Cb, Lb;         // channels [Ca, Ca + Cb): b2[b][ci - Ca][p]
  int L;                               // common (cropped) length of the virtual input == output length
};

struct BnDesc { long w, b, rm, rv, nbt, fold; int C; };

// The max of a pooled pair as torch's max_pool1d takes it: NaN when either value is NaN (fmaxf alone returns the finite partner).  For two
// finite values, or infinities, it is fmaxf.
__device__ __forceinline__ float pool_max(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }
}  // namespace

// usleep_train.hip: one layer of the training forward on plain pointers, for eegldm_usleep_layer_fwd (mode 2).  buffers: running_mean [Cout] |
// running_var [Cout] | counter; pooled, z, stat nullable.
int usleep_layer_train_entry(eegldm_ctx* ctx, const float* a, int Ca, int La, int ups, const float* b2, int Cb, int Lb, int L, const float* w,
                             const float* bias, const float* gamma, const float* beta, float* buffers, int B, int Cout, int K, float* y, float* pooled,
                             float* z, float* stat);

struct UConv { long w, b; int cin, cout, k; };
// one conv -> ELU -> BatchNorm layer of a training forward: what its backward reads (all in the arena)
struct ULayerTape {
  ConvSrc src; UConv c; int bn;
  float* z;                            // ELU output (B, cout, L): ELU' and zhat are taken from it, never from y (gamma may be 0)
  float* stat;                         // mean[cout] | rstd[cout] of the batch
  float* y;                            // BatchNorm output (B, cout, L)
  int pool_Lo;                         // encoder blocks: length after the pad + MaxPool(2), else 0
};
struct eegldm_usleep {
  eegldm_ctx* ctx = nullptr;
  eegldm_usleep_cfg cfg;
  std::vector<int> ch;
  std::vector<Entry> entries; std::vector<int> kinds;     // reference state_dict order; kind 0 = parameter, 1 = buffer
  long nparams = 0, nbuffers = 0, nfold = 0;
  float* params = nullptr; float* buffers = nullptr;
  std::vector<UConv> enc_c, pre_c, post_c; UConv bot_c, clf0, clf3, clf5;
  std::vector<BnDesc> bns;                                  // order: encoder 0..d-1, bottom, decoder i: preskip, postskip
  BnDesc* d_bns = nullptr; float* fold = nullptr; double* sums = nullptr;
  Arena arena;
  // training path (usleep_train.hip)
  float* grads = nullptr;
  std::vector<ULayerTape> tape; bool tape_valid = false;    // any other forward on this object reuses the arena: it clears tape_valid
  int tB = 0, tT = 0, tL = 0, tS = 0;                       // batch, input length, decoder output length, pooling windows of the taped forward
  const float* t_y = nullptr;                               // logits of the taped forward (the caller's buffer, or the arena)
  float* t_mh = nullptr;                                    // classifier tape: per (sample, window) mean tanh [16] | pre-ELU [16]
  int* label_flag = nullptr;                                // device: set by the loss kernel on a label >= n_classes
  long launches = 0;                                        // kernels launched by the last training call
  ~eegldm_usleep() {
    if (d_bns) (void)hipFree(d_bns); if (fold) (void)hipFree(fold); if (sums) (void)hipFree(sums); if (label_flag) (void)hipFree(label_flag);
  }
};
