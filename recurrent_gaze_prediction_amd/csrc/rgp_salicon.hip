// librgp_hip.so: the training step of the ShallowNet pre-training (SaliencyModel) around the plan's forward / backward.
// Reference: /root/reference/models/saliency_shallownet.py:246-250 (loss), :291-311 (batch + flip augmentation) and
// /root/reference/salicon_input_data.py:52-72, :123-129 (next_batch, the 1 / 255 scaling).
//
//  * rgp_salicon_batch: a whole batch gathered from a uint8 image set resident on the device -- gather by index, mirror
//    the flipped samples along the width axis, scale by float32(1 / 255) -- in ONE launch for images and maps;
//  * rgp_euclid_loss_fwd_bwd: target loss and its gradient in one pass over the maps;
//  * rgp_l2_reg: the 1e-7 regulariser over the flat parameter buffer, value and gradient in one pass.
//
// All three are HBM-streaming kernels: 16-byte loads and stores per lane wherever the alignment allows.
#include <algorithm>
#include <cstdint>

#include "image_shared.hip.h"
#include "kernels_misc.hip.h"

using namespace rgp;

namespace {

constexpr int kThreads = 256;
constexpr int kStatusBytes = 8;
constexpr int kMapSide = 49;
constexpr int kBandBytesMax = 16 * 336;                 // the largest job: 16 rows of a 112-pixel image
constexpr int kLdsBytes = kBandBytesMax + 32;           // + the source's offset within its 16-byte unit, + slack

struct SaliconParams {
  const unsigned char* images_u8;
  const unsigned char* maps_u8;
  const int* index;
  const unsigned char* flip;      // null: nothing is mirrored
  float* images;
  float* maps;
  int* status;
  int n, hw, band_rows, bands;
};

// One job = a run of whole rows of one sample (a band of its image, or its whole map): `nbytes` contiguous source bytes
// become `nbytes` contiguous floats.  The source run is copied to LDS at the same offset within a 16-byte unit it has in
// memory, so its body moves as aligned 16-byte loads (head and tail, less than 16 bytes each, as bytes); then a lane
// owns four consecutive output floats -- one 16-byte store -- and picks their bytes from LDS, pixel-mirrored within the
// row for a flipped sample.  C = bytes of a pixel (3: an RGB image, 1: a map), row = bytes of a row.
template <int C>
__device__ __forceinline__ void salicon_job(const unsigned char* __restrict__ src, float* __restrict__ dst, int nbytes, int row,
                                            bool flipped, unsigned char* lds) {
  const int tid = threadIdx.x;
  if (src) {
    const int a = (int)((uintptr_t)src & 15);                       // src - a is 16-byte aligned
    const int head = min((16 - a) & 15, nbytes), units = (nbytes - head) >> 4;
    for (int e = tid; e < head; e += kThreads) lds[a + e] = src[e];
    const uint4* s16 = (const uint4*)(src + head);
    uint4* l16 = (uint4*)(lds + a + head);                          // a + head is 0 or 16
    for (int u = tid; u < units; u += kThreads) l16[u] = s16[u];
    for (int e = head + 16 * units + tid; e < nbytes; e += kThreads) lds[a + e] = src[e];
    __syncthreads();
    lds += a;
  }
  const int pixels = row / C;
  // the byte of output element e: the same place, or the mirrored pixel of its row with the channel order kept
  auto pick = [&](int e) -> float {
    if (!src) return img::quiet_nanf();
    int at = e;
    if (flipped) {
      const int r = e / row, c = e - r * row;
      const int px = c / C, ch = c - px * C;
      at = r * row + (pixels - 1 - px) * C + ch;
    }
    return (float)lds[at] * 0.003921569f;
  };
  const int dhead = min((int)((0 - ((uintptr_t)dst >> 2)) & 3), nbytes), quads = (nbytes - dhead) >> 2;
  for (int e = tid; e < dhead; e += kThreads) dst[e] = pick(e);
  float4* d16 = (float4*)(dst + dhead);
  for (int q = tid; q < quads; q += kThreads) {
    const int e = dhead + 4 * q;
    d16[q] = make_float4(pick(e), pick(e + 1), pick(e + 2), pick(e + 3));
  }
  for (int e = dhead + 4 * quads + tid; e < nbytes; e += kThreads) dst[e] = pick(e);
}

// grid: batch * (bands + 1) workgroups; job j of a sample: j < bands an image band, j == bands the map
__global__ __launch_bounds__(kThreads) void salicon_batch_kernel(const SaliconParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kLdsBytes];
  const int jobs = p.bands + 1;
  const int s = blockIdx.x / jobs, job = blockIdx.x - s * jobs;
  const int idx = p.index[s];
  const bool ok = idx >= 0 && idx < p.n;                    // a refused index is never used as an address
  const bool flipped = p.flip && p.flip[s] != 0;
  if (!ok && job == 0 && threadIdx.x == 0) atomicAdd(p.status, 1);
  if (job < p.bands) {
    const int row = p.hw * 3;
    const long long img = (long long)p.hw * row, off = (long long)job * p.band_rows * row;
    const int nbytes = p.band_rows * row;
    salicon_job<3>(ok ? p.images_u8 + (long long)idx * img + off : nullptr, p.images + (long long)s * img + off, nbytes, row,
                   flipped, lds);
  } else {
    const int nbytes = kMapSide * kMapSide;
    salicon_job<1>(ok ? p.maps_u8 + (long long)idx * nbytes : nullptr, p.maps + (long long)s * nbytes, nbytes, kMapSide, flipped,
                   lds);
  }
}

// d[i] = (a[i] - b[i]) * scale and the block's sum of (a - b)^2: saliency_shallownet.py:248-249 and its gradient
__global__ __launch_bounds__(kThreads) void euclid_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                  float* __restrict__ d, long long n, float scale, bool vec,
                                                                  float* __restrict__ partial) {
  __shared__ float sh[kThreads / 64];
  float acc = 0.f;
  const long long tid = (long long)blockIdx.x * kThreads + threadIdx.x, nt = (long long)gridDim.x * kThreads;
  const long long quads = vec ? n >> 2 : 0;
  for (long long q = tid; q < quads; q += nt) {
    const float4 x = ((const float4*)a)[q], y = ((const float4*)b)[q];
    const float4 t = make_float4(x.x - y.x, x.y - y.y, x.z - y.z, x.w - y.w);
    acc += t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w;
    ((float4*)d)[q] = make_float4(t.x * scale, t.y * scale, t.z * scale, t.w * scale);
  }
  for (long long i = 4 * quads + tid; i < n; i += nt) {
    const float t = a[i] - b[i];
    acc += t * t;
    d[i] = t * scale;
  }
  acc = block_reduce(acc, sh, false);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// g[i] += coeff * w[i] (g null: a validation step, the value alone) and the block's sum of w^2 / 2 (tf.nn.l2_loss of every
// variable, saliency_shallownet.py:247)
constexpr int kRegThreads = 1024;
__global__ __launch_bounds__(kRegThreads) void l2_reg_partial_kernel(const float* __restrict__ w, float* __restrict__ g, long long n,
                                                                     float coeff, bool vec, float* __restrict__ partial) {
  __shared__ float sh[kRegThreads / 64];
  float acc = 0.f;
  const long long tid = (long long)blockIdx.x * kRegThreads + threadIdx.x, nt = (long long)gridDim.x * kRegThreads;
  const long long quads = vec ? n >> 2 : 0;
  for (long long q = tid; q < quads; q += nt) {
    const float4 x = ((const float4*)w)[q];
    acc += 0.5f * (x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w);
    if (g) {
      float4 y = ((float4*)g)[q];
      y.x += coeff * x.x; y.y += coeff * x.y; y.z += coeff * x.z; y.w += coeff * x.w;
      ((float4*)g)[q] = y;
    }
  }
  for (long long i = 4 * quads + tid; i < n; i += nt) {
    const float x = w[i];
    acc += 0.5f * x * x;
    if (g) g[i] += coeff * x;
  }
  acc = block_reduce(acc, sh, false);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// out = scale * (partial[0] + partial[1] + ...), in that order
__global__ void scaled_sum_kernel(const float* __restrict__ partial, int n, float scale, float* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += partial[i];
    *out = s * scale;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

size_t rgp_salicon_workspace_bytes(void) { return kStatusBytes; }

int rgp_salicon_batch(const rgp_salicon_batch_args* a, rgp_stream_t stream) {
  RGP_REQUIRE(a != nullptr, "rgp_salicon_batch: args is NULL");
  RGP_REQUIRE(a->images != nullptr, "rgp_salicon_batch: images (output) is NULL");
  RGP_REQUIRE(a->maps != nullptr, "rgp_salicon_batch: maps (output) is NULL");
  RGP_REQUIRE(a->batch >= 0, "rgp_salicon_batch: batch %d is negative", a->batch);
  RGP_REQUIRE(a->h == a->w, "rgp_salicon_batch: h %d != w %d", a->h, a->w);
  RGP_REQUIRE(a->h == 98 || a->h == 112, "rgp_salicon_batch: h %d (98 or 112)", a->h);
  RGP_REQUIRE(a->map_h == kMapSide && a->map_w == kMapSide, "rgp_salicon_batch: map_h x map_w %d x %d (49 x 49)", a->map_h,
              a->map_w);
  RGP_REQUIRE(a->n > 0, "rgp_salicon_batch: n %d", a->n);
  RGP_REQUIRE(a->images_u8 != nullptr, "rgp_salicon_batch: images_u8 is NULL");
  RGP_REQUIRE(a->maps_u8 != nullptr, "rgp_salicon_batch: maps_u8 is NULL");
  RGP_REQUIRE(a->index != nullptr, "rgp_salicon_batch: index is NULL");
  RGP_REQUIRE(a->workspace != nullptr && ((uintptr_t)a->workspace & 7) == 0, "rgp_salicon_batch: workspace is NULL or not 8-byte aligned");
  RGP_REQUIRE(a->workspace_bytes >= (size_t)kStatusBytes, "rgp_salicon_batch: workspace_bytes %zu < %d", a->workspace_bytes,
              kStatusBytes);
  RGP_REQUIRE(((uintptr_t)a->images & 3) == 0 && ((uintptr_t)a->maps & 3) == 0, "rgp_salicon_batch: images / maps not 4-byte aligned");
  if (a->batch == 0) return RGP_OK;
  SaliconParams p;
  p.images_u8 = a->images_u8; p.maps_u8 = a->maps_u8; p.index = a->index; p.flip = a->flip;
  p.images = a->images; p.maps = a->maps; p.status = (int*)a->workspace;
  p.n = a->n; p.hw = a->h;
  p.band_rows = a->h == 98 ? 14 : 16;                       // 7 bands either way; 14 * 294 and 16 * 336 bytes <= kBandBytesMax
  p.bands = a->h / p.band_rows;
  static_assert(14 * 294 <= kBandBytesMax && 16 * 336 <= kBandBytesMax && kMapSide * kMapSide <= kBandBytesMax, "LDS image");
  RGP_REQUIRE((long long)a->batch * (p.bands + 1) < (1ll << 31), "rgp_salicon_batch: batch %d too large", a->batch);
  hipStream_t s = (hipStream_t)stream;
  RGP_HIP(hipMemsetAsync(a->workspace, 0, kStatusBytes, s));
  hipLaunchKernelGGL(salicon_batch_kernel, dim3(a->batch * (p.bands + 1)), dim3(kThreads), 0, s, p);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

int rgp_salicon_status(const void* workspace, int* refused_out, rgp_stream_t stream) {
  int refused;
  RGP_TRY(img::read_status("rgp_salicon_status", workspace, refused_out, stream, &refused));
  RGP_REQUIRE(refused == 0, "rgp_salicon_batch: %d sample(s) refused (an index entry outside [0, n)): NaN in images and maps", refused);
  return RGP_OK;
}

int rgp_euclid_loss_fwd_bwd(const float* maps, const float* labels, long long n, float scale, float* workspace, float* loss,
                            float* d_maps, rgp_stream_t stream) {
  RGP_REQUIRE(maps != nullptr, "rgp_euclid_loss_fwd_bwd: maps is NULL");
  RGP_REQUIRE(labels != nullptr, "rgp_euclid_loss_fwd_bwd: labels is NULL");
  RGP_REQUIRE(n > 0, "rgp_euclid_loss_fwd_bwd: n %lld", n);
  RGP_REQUIRE(workspace != nullptr, "rgp_euclid_loss_fwd_bwd: workspace is NULL");
  RGP_REQUIRE(loss != nullptr, "rgp_euclid_loss_fwd_bwd: loss is NULL");
  RGP_REQUIRE(d_maps != nullptr, "rgp_euclid_loss_fwd_bwd: d_maps is NULL");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = aligned16(maps) && aligned16(labels) && aligned16(d_maps);
  euclid_partial_kernel<<<RGP_SQNORM_PARTIALS, kThreads, 0, s>>>(maps, labels, d_maps, n, scale, vec, workspace);
  scaled_sum_kernel<<<1, 64, 0, s>>>(workspace, RGP_SQNORM_PARTIALS, 0.5f * scale, loss);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

int rgp_l2_reg(const float* params, float* grads, long long n, float coeff, float* workspace, float* reg_loss, rgp_stream_t stream) {
  RGP_REQUIRE(params != nullptr, "rgp_l2_reg: params is NULL");
  RGP_REQUIRE(n > 0, "rgp_l2_reg: n %lld", n);
  RGP_REQUIRE(workspace != nullptr, "rgp_l2_reg: workspace is NULL");
  RGP_REQUIRE(reg_loss != nullptr, "rgp_l2_reg: reg_loss is NULL");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = aligned16(params) && aligned16(grads);
  l2_reg_partial_kernel<<<RGP_SQNORM_PARTIALS, kRegThreads, 0, s>>>(params, grads, n, coeff, vec, workspace);
  scaled_sum_kernel<<<1, 64, 0, s>>>(workspace, RGP_SQNORM_PARTIALS, coeff, reg_loss);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

}  // extern "C"
