// librgp_hip.so: the loader's frame images (include/rgp.h, "loader frame images"): crc_input_data_seq.py:186-209 --
// Image.resize((w, h), Image.ANTIALIAS) on selected uint8 RGB frames, then * float32(1 / 255) -- in ONE launch.
//
// Pillow's 8-bit resample is two passes of 22-bit fixed-point sums with host-made tables: horizontal on the input rows
// the vertical tables touch, then vertical on the 8-bit result.  A workgroup owns (output frame, band of output rows):
//   1. it checks the frame index and both bounds tables (nothing unchecked addresses memory), and stages in LDS the
//      horizontal weights TRANSPOSED ([tap][xx]: lanes run along xx, so a tap's weights are one conflict-free row),
//      the band's vertical weights and bounds;
//   2. it streams the band's input rows [ya, yb) through a staging area of kStageBytes: the rows of a chunk are
//      contiguous in memory, so the chunk is copied as 16-byte words from the aligned address below its first byte
//      (rows of W * 3 bytes and frames at odd addresses leave only a byte offset `mis` into the staging area); the next
//      chunk's words are loaded into registers before the current one is resampled;
//   3. horizontal: a work item is (xx, four input rows): per four taps it reads four weights and, per row, four dwords
//      that v_alignbyte turns into the twelve bytes of four RGB pixels -- dword LDS reads, unpacked in registers --
//      and makes 48 24-bit multiply-adds into 12 int32 sums; the clamped bytes go to the band's 8-bit image in LDS;
//   4. vertical from that image, a work item being (output row, dword of the row): four sums per LDS read;
//   5. the band's output bytes are collected in the staging area and stored coalesced: fp32 (u8 * 0.003921569f) and /
//      or uint8 (aligned dwords, bytes at the two ends).
// A skipped pass (in == out) copies.  Sums are int32 and exact (the host builder bounds sum|k|), so the bits do not
// depend on the banding.  No float before the final scale, no scratch.
#include <climits>
#include <cstdint>

#include "image_shared.hip.h"

using namespace rgp;
using namespace rgp::img;

namespace {

constexpr int kThreads = 256;
constexpr int kStageBytes = RGP_FRAMES_STAGE_BYTES;
constexpr int kStageSlack = 64;                       // reads of the last taps' dwords run a few bytes past a chunk
constexpr int kPrefetch = kStageBytes / (kThreads * 16);
constexpr int kRowsPerItem = 4;
constexpr int kHeadBytes = 16 + 2 * RGP_FRAMES_MAX_OUT * 4;   // the flag, then per band the first and last input row
static_assert(kPrefetch * kThreads * 16 == kStageBytes, "a chunk is kPrefetch 16-byte words per thread");
static_assert((kStageBytes - 16) / (RGP_FRAMES_MAX_IN_W * 3) >= kRowsPerItem, "four rows of the widest frame fit a chunk");
static_assert(RGP_FRAMES_LDS_BYTES <= 160 * 1024, "LDS of a CU");

struct FramesParams {
  const unsigned char* frames;
  const int *frame_index, *kh, *bh, *kv, *bv;
  float* images;
  unsigned char* images_u8;
  int* status;
  int n_frames, fh, fw, n_out, out_h, out_w, ksize_h, ksize_v, bands;
  int mid_rows, band_rows;                       // what the LDS image / the vertical tables of a band hold
  int off_mid, off_kt, off_bh, off_kv, off_bv;   // byte offsets into the dynamic LDS
};

struct Layout {
  int bands, band_rows, mid_rows, pitch_mid, kt_rows;
  int off_mid, off_kt, off_bh, off_kv, off_bv, total;
};

// LDS of a workgroup when the out_h rows are cut into nb bands; false if the band's output image exceeds the staging area
bool layout_for(int fh, int fw, int out_h, int out_w, int ksize_h, int ksize_v, int nb, Layout* L) {
  const bool hpass = fw != out_w, vpass = fh != out_h;
  L->bands = nb;
  L->band_rows = (out_h + nb - 1) / nb;
  // input rows of a band: yb - ya < (band_rows - 1) in / out + 2 support + 1 <= (band_rows - 1) in / out + ksize
  L->mid_rows = vpass ? std::min<long long>(fh, (long long)(L->band_rows - 1) * fh / out_h + ksize_v + 2) : L->band_rows;
  L->pitch_mid = align_i(out_w * 3, 4);
  L->kt_rows = align_i(ksize_h, 4);
  int off = kHeadBytes;
  off = align_i(off, 16) + kStageBytes + kStageSlack;
  L->off_mid = off = align_i(off, 16);
  off += L->mid_rows * L->pitch_mid + 16;
  L->off_kt = off = align_i(off, 16);
  if (hpass) off += L->kt_rows * out_w * 4;
  L->off_bh = off;
  if (hpass) off += out_w * 8;
  L->off_kv = off;
  if (vpass) off += L->band_rows * ksize_v * 4;
  L->off_bv = off = align_i(off, 8);
  if (vpass) off += L->band_rows * 8;
  L->total = align_i(off, 16);
  return L->band_rows * out_w * 3 <= kStageBytes;
}

bool geometry_ok(int fh, int fw, int out_h, int out_w, int ksize_h, int ksize_v) {
  if (fh < 1 || fw < 1 || fw > RGP_FRAMES_MAX_IN_W || out_h < 1 || out_w < 1 || out_h > RGP_FRAMES_MAX_OUT || out_w > RGP_FRAMES_MAX_OUT)
    return false;
  if (fw != out_w && (ksize_h < 1 || ksize_h > RGP_FRAMES_MAX_KSIZE)) return false;
  if (fh != out_h && (ksize_v < 1 || ksize_v > RGP_FRAMES_MAX_KSIZE)) return false;
  return true;
}

// bands = 0.  A band re-reads about ksize_v input rows, so the count starts at what gives two workgroups per CU but not
// past bands of ksize_v input rows (the re-read no larger than the band), and then goes up to the least count whose
// workgroup leaves room for a second one on its CU (RGP_FRAMES_LDS_TARGET), not past bands of 2 ksize_v input rows.
// Otherwise, and for a caller's count: the least count >= the request whose workgroup fits RGP_FRAMES_LDS_BYTES.
bool plan(int fh, int fw, int out_h, int out_w, int ksize_h, int ksize_v, int n_out, int bands, Layout* L) {
  int first = bands;
  if (bands == 0) {
    const bool vpass = fh != out_h;
    const int fill = (512 + std::max(n_out, 1) - 1) / std::max(n_out, 1);
    first = std::max(1, std::min({out_h, fill, vpass ? fh / ksize_v : out_h}));
    const int most = std::max(first, vpass ? std::min(out_h, fh / (2 * ksize_v)) : out_h);
    for (int nb = first; nb <= most; ++nb)
      if (layout_for(fh, fw, out_h, out_w, ksize_h, ksize_v, nb, L) && L->total <= RGP_FRAMES_LDS_TARGET) return true;
  }
  for (int nb = std::max(first, 1); nb <= out_h; ++nb)
    if (layout_for(fh, fw, out_h, out_w, ksize_h, ksize_v, nb, L) && L->total <= RGP_FRAMES_LDS_BYTES) return true;
  return false;
}

__device__ __forceinline__ int band_of_row(int r, int nb, int out_h) { return ((r + 1) * nb - 1) / out_h; }

__device__ __forceinline__ int mad24(unsigned byte, int k, int acc) { return __mul24((int)byte, k) + acc; }

// the band's bytes [e0, e0 + n_bytes) of both outputs from the LDS bytes `src` (null: a refused frame, NaN and 0)
__device__ __forceinline__ void store_band(const FramesParams& p, const unsigned char* src, long long e0, int n_bytes, int tid) {
  if (p.images) {
    float* dst = p.images + e0;
    for (int e = tid; e < n_bytes; e += kThreads) dst[e] = src ? (float)src[e] * 0.003921569f : quiet_nanf();
  }
  if (p.images_u8) store_lds_bytes<kThreads>(p.images_u8 + e0, src, n_bytes, tid);
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// rows [y, y + chunk_rows) of the band's input, as 16-byte words from the aligned address below the first byte
__device__ __forceinline__ void fetch_chunk(const unsigned char* fp, int y, int chunk_rows, int rows_in, int W3, int tid,
                                            u32x4 (&pf)[kPrefetch], int& mis, int& n16) {
  const int rc = min(chunk_rows, rows_in - y);
  const unsigned char* g = fp + (long long)y * W3;
  mis = (int)((uintptr_t)g & 15);
  n16 = rc > 0 ? (mis + rc * W3 + 15) >> 4 : 0;
  const u32x4* g16 = (const u32x4*)(g - mis);
#pragma unroll
  for (int j = 0; j < kPrefetch; ++j) {
    const int i = tid + j * kThreads;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (i < n16) v = g16[i];
    pf[j] = v;
  }
}

__global__ __launch_bounds__(kThreads) void frame_images_kernel(const FramesParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  int* sBad = (int*)lds;
  int* sLo = (int*)(lds + 16);
  int* sHi = sLo + RGP_FRAMES_MAX_OUT;
  unsigned char* sStage = lds + (kHeadBytes + 15) / 16 * 16;
  const unsigned* sStage32 = (const unsigned*)sStage;
  unsigned char* sMid = lds + p.off_mid;
  unsigned* sMid32 = (unsigned*)sMid;
  int* sKT = (int*)(lds + p.off_kt);
  int2* sBh = (int2*)(lds + p.off_bh);
  int* sKv = (int*)(lds + p.off_kv);
  int2* sBv = (int2*)(lds + p.off_bv);

  const int tid = threadIdx.x;
  const int f = blockIdx.x / p.bands, band = blockIdx.x - f * p.bands;
  const int out_h = p.out_h, out_w = p.out_w, fh = p.fh, fw = p.fw, nb = p.bands;
  const bool hpass = fw != out_w, vpass = fh != out_h;
  const int r0 = band * out_h / nb, r1 = (band + 1) * out_h / nb, br = r1 - r0;
  const int W3 = fw * 3, O3 = out_w * 3, pw = (O3 + 3) >> 2, pitch_mid = pw * 4;
  const long long e0 = ((long long)f * out_h + r0) * O3;

  // ---- 1. every value that will address memory is checked first; all bands of a frame come to the same verdict
  if (tid == 0) *sBad = 0;
  for (int b = tid; b < nb; b += kThreads) { sLo[b] = INT_MAX; sHi[b] = 0; }
  __syncthreads();
  const int src = p.frame_index ? p.frame_index[f] : f;
  bool bad = src < 0 || src >= p.n_frames;
  if (hpass)
    for (int xx = tid; xx < out_w; xx += kThreads) sBh[xx] = checked_bounds(p.bh, xx, p.ksize_h, fw, bad);
  if (vpass)
    for (int r = tid; r < out_h; r += kThreads) {
      bool row_bad = false;
      const int2 by = checked_bounds(p.bv, r, p.ksize_v, fh, row_bad);
      if (row_bad) { bad = true; continue; }
      const int b = band_of_row(r, nb, out_h);
      atomicMin(&sLo[b], by.x);
      atomicMax(&sHi[b], by.x + by.y);
    }
  if (bad) atomicOr(sBad, 1);
  __syncthreads();
  if (vpass)
    for (int b = tid; b < nb; b += kThreads)
      if (sHi[b] - sLo[b] > p.mid_rows) atomicOr(sBad, 1);   // (a row that failed above left its band's pair alone)
  __syncthreads();
  if (*sBad != 0) {
    store_band(p, nullptr, e0, br * O3, tid);
    if (band == 0 && tid == 0) atomicAdd(p.status, 1);
    return;
  }
  const int ya = vpass ? sLo[band] : r0, yb = vpass ? sHi[band] : r1;
  const int rows_in = max(yb - ya, 0);

  // ---- the tables of this band
  if (hpass) stage_weights_transposed<kThreads>(sKT, p.kh, sBh, out_w, p.ksize_h, (p.ksize_h + 3) & ~3, tid);   // four taps a step
  if (vpass) {
    for (int rr = tid; rr < br; rr += kThreads) sBv[rr] = make_int2(p.bv[2 * (r0 + rr)] - ya, p.bv[2 * (r0 + rr) + 1]);
    for (int i = tid; i < br * p.ksize_v; i += kThreads) {
      const int rr = i / p.ksize_v, t = i - rr * p.ksize_v;
      sKv[i] = t < p.bv[2 * (r0 + rr) + 1] ? p.kv[(r0 + rr) * p.ksize_v + t] : 0;
    }
  }
  __syncthreads();

  // ---- 2. / 3. the input rows [ya, yb), a chunk of whole rows at a time
  const unsigned char* fp = p.frames + (long long)src * fh * W3 + (long long)ya * W3;
  const int chunk_rows = min(((kStageBytes - 16) / W3) & ~(kRowsPerItem - 1), 64);
  u32x4 pf[kPrefetch];
  int mis = 0, n16 = 0;
  fetch_chunk(fp, 0, chunk_rows, rows_in, W3, tid, pf, mis, n16);
  for (int y = 0; y < rows_in; y += chunk_rows) {
    const int rc = min(chunk_rows, rows_in - y), cur_mis = mis;
#pragma unroll
    for (int j = 0; j < kPrefetch; ++j) {
      const int i = tid + j * kThreads;
      if (i < n16) ((u32x4*)sStage)[i] = pf[j];
    }
    __syncthreads();
    fetch_chunk(fp, y + chunk_rows, chunk_rows, rows_in, W3, tid, pf, mis, n16);
    if (hpass) {
      const int groups = (rc + kRowsPerItem - 1) / kRowsPerItem;
      for (int item = tid; item < groups * out_w; item += kThreads) {
        const int g = item / out_w, xx = item - g * out_w;
        const int2 bx = sBh[xx];
        int w[kRowsPerItem], sh[kRowsPerItem], acc[kRowsPerItem][3];
#pragma unroll
        for (int q = 0; q < kRowsPerItem; ++q) {
          const int row = min(g * kRowsPerItem + q, rc - 1);   // a row past the chunk repeats the last one; not stored
          const int o = cur_mis + row * W3 + bx.x * 3;
          w[q] = o >> 2;
          sh[q] = o & 3;
          acc[q][0] = acc[q][1] = acc[q][2] = 0;
        }
        for (int t0 = 0; t0 < bx.y; t0 += 4) {
          const int* kt = sKT + t0 * out_w + xx;
          const int c0 = kt[0], c1 = kt[out_w], c2 = kt[2 * out_w], c3 = kt[3 * out_w];
          const int step = 3 * (t0 >> 2);
#pragma unroll
          for (int q = 0; q < kRowsPerItem; ++q) {
            const unsigned* s = sStage32 + w[q] + step;
            const unsigned d0 = s[0], d1 = s[1], d2 = s[2], d3 = s[3];
            const unsigned u0 = __builtin_amdgcn_alignbyte(d1, d0, sh[q]), u1 = __builtin_amdgcn_alignbyte(d2, d1, sh[q]),
                           u2 = __builtin_amdgcn_alignbyte(d3, d2, sh[q]);
            // u0 = r0 g0 b0 r1, u1 = g1 b1 r2 g2, u2 = b2 r3 g3 b3 (lowest byte first)
            acc[q][0] = mad24(u0 & 255u, c0, acc[q][0]);
            acc[q][1] = mad24((u0 >> 8) & 255u, c0, acc[q][1]);
            acc[q][2] = mad24((u0 >> 16) & 255u, c0, acc[q][2]);
            acc[q][0] = mad24(u0 >> 24, c1, acc[q][0]);
            acc[q][1] = mad24(u1 & 255u, c1, acc[q][1]);
            acc[q][2] = mad24((u1 >> 8) & 255u, c1, acc[q][2]);
            acc[q][0] = mad24((u1 >> 16) & 255u, c2, acc[q][0]);
            acc[q][1] = mad24(u1 >> 24, c2, acc[q][1]);
            acc[q][2] = mad24(u2 & 255u, c2, acc[q][2]);
            acc[q][0] = mad24((u2 >> 8) & 255u, c3, acc[q][0]);
            acc[q][1] = mad24((u2 >> 16) & 255u, c3, acc[q][1]);
            acc[q][2] = mad24(u2 >> 24, c3, acc[q][2]);
          }
        }
#pragma unroll
        for (int q = 0; q < kRowsPerItem; ++q) {
          const int row = g * kRowsPerItem + q;
          if (row < rc) {
            unsigned char* m = sMid + (y + row) * pitch_mid + xx * 3;
            m[0] = (unsigned char)clip8(acc[q][0]);
            m[1] = (unsigned char)clip8(acc[q][1]);
            m[2] = (unsigned char)clip8(acc[q][2]);
          }
        }
      }
    } else {   // in == out: the row's bytes, realigned to the image's dwords
      for (int item = tid; item < rc * pw; item += kThreads) {
        const int row = item / pw, j = item - row * pw;
        const int o = cur_mis + row * W3 + 4 * j;
        sMid32[(y + row) * pw + j] = __builtin_amdgcn_alignbyte(sStage32[(o >> 2) + 1], sStage32[o >> 2], o & 3);
      }
    }
    __syncthreads();
  }

  // ---- 4. vertical, from the band's 8-bit image into the band's output bytes (the staging area is free now)
  for (int item = tid; item < br * pw; item += kThreads) {
    const int rr = item / pw, j = item - rr * pw;
    // The four bytes stay four values up to their stores.  Packed as clip8(a0) | clip8(a1) << 8 | ..., hipcc (ROCm 7.2)
    // forms the low half with v_ashr_pk_u8_i32 and ORs the other two bytes into its result, and on the device bytes 2 and
    // 3 then came out with further bits set: nothing here relies on the upper half of that instruction's result.
    int b0, b1, b2, b3;
    if (vpass) {
      const int2 by = sBv[rr];
      const unsigned* m = sMid32 + by.x * pw + j;
      const int* k = sKv + rr * p.ksize_v;
      int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
      for (int t = 0; t < by.y; ++t) {
        const unsigned d = m[t * pw];
        const int c = k[t];
        a0 = mad24(d & 255u, c, a0);
        a1 = mad24((d >> 8) & 255u, c, a1);
        a2 = mad24((d >> 16) & 255u, c, a2);
        a3 = mad24(d >> 24, c, a3);
      }
      b0 = clip8(a0); b1 = clip8(a1); b2 = clip8(a2); b3 = clip8(a3);
    } else {
      const unsigned d = sMid32[rr * pw + j];
      b0 = d & 255u; b1 = (d >> 8) & 255u; b2 = (d >> 16) & 255u; b3 = d >> 24;
    }
    unsigned char* o = sStage + rr * O3 + 4 * j;
    if (4 * j + 0 < O3) o[0] = (unsigned char)b0;
    if (4 * j + 1 < O3) o[1] = (unsigned char)b1;
    if (4 * j + 2 < O3) o[2] = (unsigned char)b2;
    if (4 * j + 3 < O3) o[3] = (unsigned char)b3;
  }
  __syncthreads();

  // ---- 5. both outputs, coalesced
  store_band(p, sStage, e0, br * O3, tid);
}

}  // namespace

extern "C" {

size_t rgp_frames_workspace_bytes(void) { return kStatusBytes; }

int rgp_frames_plan(int fh, int fw, int out_h, int out_w, int ksize_h, int ksize_v, int n_out, int bands, int* lds_bytes,
                    int* mid_rows) {
  Layout L;
  if (lds_bytes) *lds_bytes = 0;
  if (mid_rows) *mid_rows = 0;
  if (!geometry_ok(fh, fw, out_h, out_w, ksize_h, ksize_v) || n_out < 0 || bands < 0 || bands > out_h) return 0;
  if (!plan(fh, fw, out_h, out_w, ksize_h, ksize_v, n_out, bands, &L)) return 0;
  if (lds_bytes) *lds_bytes = L.total;
  if (mid_rows) *mid_rows = L.mid_rows;
  return L.bands;
}

int rgp_frame_images(const rgp_frames_args* a, rgp_stream_t stream) {
  RGP_REQUIRE(a != nullptr, "rgp_frame_images: args is NULL");
  RGP_REQUIRE(a->n_out >= 0, "rgp_frame_images: n_out = %d must not be negative", a->n_out);
  if (a->n_out == 0) return RGP_OK;
  RGP_REQUIRE(a->n_frames >= 0, "rgp_frame_images: n_frames = %d must not be negative", a->n_frames);
  RGP_REQUIRE(a->fh >= 1 && a->fw >= 1, "rgp_frame_images: fh = %d and fw = %d must be at least 1", a->fh, a->fw);
  RGP_REQUIRE(a->fw <= RGP_FRAMES_MAX_IN_W, "rgp_frame_images: fw = %d above RGP_FRAMES_MAX_IN_W = %d", a->fw, RGP_FRAMES_MAX_IN_W);
  RGP_REQUIRE(a->out_h >= 1 && a->out_h <= RGP_FRAMES_MAX_OUT, "rgp_frame_images: out_h = %d must be in [1, RGP_FRAMES_MAX_OUT = %d]",
              a->out_h, RGP_FRAMES_MAX_OUT);
  RGP_REQUIRE(a->out_w >= 1 && a->out_w <= RGP_FRAMES_MAX_OUT, "rgp_frame_images: out_w = %d must be in [1, RGP_FRAMES_MAX_OUT = %d]",
              a->out_w, RGP_FRAMES_MAX_OUT);
  const bool hpass = a->fw != a->out_w, vpass = a->fh != a->out_h;
  const char* cap = "RGP_FRAMES_MAX_KSIZE";
  if (hpass) RGP_TRY(require_pass("rgp_frame_images", 'h', a->ksize_h, a->kh, a->bh, "fw", a->fw, a->out_w, cap, RGP_FRAMES_MAX_KSIZE));
  if (vpass) RGP_TRY(require_pass("rgp_frame_images", 'v', a->ksize_v, a->kv, a->bv, "fh", a->fh, a->out_h, cap, RGP_FRAMES_MAX_KSIZE));
  RGP_REQUIRE(a->bands >= 0 && a->bands <= a->out_h, "rgp_frame_images: bands = %d must be in [0, out_h = %d]", a->bands, a->out_h);
  RGP_REQUIRE(a->images || a->images_u8, "rgp_frame_images: images and images_u8 are both NULL: nothing to compute");
  RGP_REQUIRE((long long)a->n_frames * a->fh * a->fw * 3 < RGP_FRAMES_MAX_BYTES,
              "rgp_frame_images: n_frames = %d frames of %d x %d x 3 bytes: RGP_FRAMES_MAX_BYTES = 2^40 or more", a->n_frames, a->fh, a->fw);
  RGP_REQUIRE((long long)a->n_out * a->out_h * a->out_w * 3 < RGP_FRAMES_MAX_BYTES,
              "rgp_frame_images: n_out = %d images of %d x %d x 3: RGP_FRAMES_MAX_BYTES = 2^40 or more", a->n_out, a->out_h, a->out_w);
  RGP_REQUIRE(a->frames != nullptr, "rgp_frame_images: frames is NULL");
  RGP_REQUIRE(a->n_frames >= 1, "rgp_frame_images: n_frames = 0 and n_out = %d", a->n_out);
  RGP_REQUIRE(((size_t)a->images & 3) == 0, "rgp_frame_images: images must be 4-byte aligned");
  RGP_TRY(require_workspace("rgp_frame_images", a->workspace, a->workspace_bytes, kStatusBytes));
  Layout L;
  RGP_REQUIRE(plan(a->fh, a->fw, a->out_h, a->out_w, hpass ? a->ksize_h : 0, vpass ? a->ksize_v : 0, a->n_out, a->bands, &L),
              "rgp_frame_images: %d x %d -> %d x %d with ksize_h = %d, ksize_v = %d: not even one output row per band fits "
              "RGP_FRAMES_LDS_BYTES = %d", a->fh, a->fw, a->out_h, a->out_w, a->ksize_h, a->ksize_v, RGP_FRAMES_LDS_BYTES);
  RGP_REQUIRE((long long)a->n_out * L.bands <= INT_MAX,
              "rgp_frame_images: n_out = %d images in %d bands need more than 2^31 - 1 workgroups: split the call", a->n_out, L.bands);

  FramesParams p{};
  p.frames = a->frames; p.frame_index = a->frame_index;
  p.kh = a->kh; p.bh = a->bh; p.kv = a->kv; p.bv = a->bv;
  p.images = a->images; p.images_u8 = a->images_u8;
  p.status = (int*)a->workspace;
  p.n_frames = a->n_frames; p.fh = a->fh; p.fw = a->fw; p.n_out = a->n_out; p.out_h = a->out_h; p.out_w = a->out_w;
  p.ksize_h = hpass ? a->ksize_h : 0; p.ksize_v = vpass ? a->ksize_v : 0;
  p.bands = L.bands; p.mid_rows = L.mid_rows; p.band_rows = L.band_rows;
  p.off_mid = L.off_mid; p.off_kt = L.off_kt; p.off_bh = L.off_bh; p.off_kv = L.off_kv; p.off_bv = L.off_bv;
  hipStream_t s = (hipStream_t)stream;
  RGP_TRY(ensure_dyn_smem((const void*)frame_images_kernel, RGP_FRAMES_LDS_BYTES));
  RGP_TRY(clear_status(a->workspace, s));
  hipLaunchKernelGGL(frame_images_kernel, dim3(a->n_out * L.bands), dim3(kThreads), L.total, s, p);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

int rgp_frames_status(const void* workspace, int* refused_out, rgp_stream_t stream) {
  int refused;
  RGP_TRY(read_status("rgp_frames_status", workspace, refused_out, stream, &refused));
  RGP_REQUIRE(refused == 0,
              "rgp_frame_images: %d output frame(s) refused (a frame_index entry outside [0, n_frames), or a bounds table entry "
              "out of range): NaN in images, 0 in images_u8", refused);
  return RGP_OK;
}

}  // extern "C"
