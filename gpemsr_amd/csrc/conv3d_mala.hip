// The MALA 3-D U-Net of the segmentation step (gpemsr_amd/affinity_mala.py): valid 3x3x3 convolutions on the f32 matrix pipe, its fused
// decoder merge, the (1, 3, 3) max pool and the last-wins window placement of the sliding-window inference.
//
// All products are exact f32 on v_mfma_f32_16x16x4_f32 (one rounding per product, guide section 3); only the summation order differs from
// the reference's.  Activations are NDHWC float32 ([B, D, H, W, C], channels fastest, a per-voxel stride `ld`).
//
// gpemsr_conv3d_valid_thin -- cout <= 80 (conv1-4, conv13/14, conv16/17).  The halo-in-LDS design of gpemsr_conv3d (csrc/conv3d.hip) in a
//   valid form: output (d-2, h-2, w-2), the halo anchored at the output voxel (no padding, no zero fill).  Workgroup tile 2 x 8 x 16 output
//   voxels; each wave owns one slice x 4 rows x 16 columns as four 16-voxel M blocks of 4 x 4 (y, x) voxels, so every extent that is a
//   multiple of 4 (84, 56, 20 ...) leaves only whole M blocks past the edge, and those blocks (and a wave whose 4 rows are all past the edge)
//   skip their MFMAs.  B (the packed weights, <= 130 KB per layer here) is read from L1 / L2 per tap as in gpemsr_conv3d.
//
// gpemsr_conv3d_valid_wide -- any cout (used for 300 / 1500: conv5-8, conv10/11).  Implicit GEMM, M = output voxels linearised over
//   (image, z, y, x), N = cout, K = 27 taps x cin.  Workgroup tile 128 voxels x (16 NJ) couts, 4 waves of 32 voxels x 16 NJ couts; K runs in
//   chunks of (one tap, 16 channels): the A chunk is 128 contiguous NDHWC runs of 16 channels, the B chunk 16 rows of the packed
//   [tap][cin][coutp] weight.  Both are staged in LDS and double-buffered (the next chunk's global loads are in flight while the current one
//   is multiplied; one barrier per chunk).  N is cut into 64-wide tiles plus one tail launch of 16 .. 64 (cout < 64 is the tail alone), so cout 300 and 1500 execute
//   304 and 1504 columns (the 128-wide tile would execute 384 for 300).  Where the tile grid would leave CUs idle (conv7 / conv8 / conv10 /
//   conv11 on a 4 x 4 .. 10 x 10 plane) K is split over up to 16 workgroups that write partial sums; a second kernel adds them in split
//   order (deterministic), then bias and activation.  The split follows one image's geometry, so results do not depend on the batch size.
//
// gpemsr_mala_merge -- mc = conv1x1(ConvTranspose3d((1,3,3), stride (1,3,3), groups=C)(x)) + bias + crop(skip).  The transposed
//   convolution's stride equals its kernel, so each of its outputs is the single product x[c] * wt[c][i][j]; that product is formed while A is
//   staged (bit-identical to the reference's dconv output) and the 9x-upsampled tensor is never materialised.  The GEMM runs at the low
//   resolution with N = 9 sub-positions x cout (the wide kernel's machinery, one tap), and the epilogue stores pixel-shuffled:
//   out[z][3y+i][3x+j][n] = (sum + bias[n]) + skip[z+cz][3y+i+c][3x+j+c][n].
#include "common.h"

namespace gpemsr {

typedef float f32x4m __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float mala_act(float v, int act) {
  if (act == GPEMSR_ACT_LRELU_005) return v > 0.f ? v : v * 0.005f;
  return apply_act(v, act);
}

// ------------------------------------------------------------------------------------------------------------------------------- thin
constexpr int MT_TW = 16, MT_TH = 8, MT_TZ = 2, MT_CK = 16, MT_CKP = 18;
constexpr int MT_HZ = MT_TZ + 2, MT_HY = MT_TH + 2, MT_HX = MT_TW + 2, MT_HVOX = MT_HZ * MT_HY * MT_HX;

struct ThinParams {
  const float* in; int in_ld; long long in_istride;
  int d, h, w, od, oh, ow, cin, cout, ks4;
  const float* wp; const float* bias;
  float* out; int out_ld; long long out_istride;
  int act, tiles_x, tiles_y, tiles_z;
};

template <int NT>
__global__ __launch_bounds__(256, 2) void conv3d_valid_thin_kernel(ThinParams P) {
  __shared__ float As[MT_HVOX * MT_CKP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int b = blockIdx.x;
  const int tx = b % P.tiles_x; b /= P.tiles_x;
  const int ty = b % P.tiles_y; b /= P.tiles_y;
  const int tz = b % P.tiles_z;
  const int img = b / P.tiles_z;
  const int x0 = tx * MT_TW, y0 = ty * MT_TH, z0 = tz * MT_TZ;
  const float* in = P.in + img * P.in_istride;
  const int wz = wave >> 1, wy = (wave & 1) * 4, li = lane & 15, lk = lane >> 4;
  // M blocks of this wave that hold at least one output voxel (wave-uniform): rows wy.. are 4 voxels tall, blocks 4 voxels wide
  const bool live = (z0 + wz < P.od) && (y0 + wy < P.oh);
  const int mact = live ? min(4, (P.ow - x0 + 3) >> 2) : 0;

  f32x4m acc[4][NT];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[m][j] = f32x4m{0.f, 0.f, 0.f, 0.f};

  const long long tap_stride = (long long)P.ks4 * NT * 64;
  // lane i of an M block: voxel (dy, dx) = (i >> 2, i & 3) of the block's 4 x 4 patch
  const int lane_off = ((wz * MT_HY + wy + (li >> 2)) * MT_HX + (li & 3)) * MT_CKP;
  for (int c0 = 0; c0 < P.cin; c0 += MT_CK) {
    const int cc = min(MT_CK, P.cin - c0);
    const int nst = (cc + 3) >> 2, cc4 = nst * 4;
    __syncthreads();
    for (int e = tid; e < MT_HVOX * cc4; e += 256) {
      const int v = e / cc4, c = e - v * cc4;
      const int hx = v % MT_HX, t = v / MT_HX, hy = t % MT_HY, hz = t / MT_HY;
      const int gz = z0 + hz, gy = y0 + hy, gx = x0 + hx;
      float val = 0.f;   // channels past cin must be 0 (they meet zero weights); voxels past the input only feed outputs never stored
      if (c < cc && gz < P.d && gy < P.h && gx < P.w) val = in[(((long long)gz * P.h + gy) * P.w + gx) * P.in_ld + c0 + c];
      As[v * MT_CKP + c] = val;
    }
    __syncthreads();
    if (mact == 0) continue;
    const float* wchunk = P.wp + (long long)(c0 >> 2) * NT * 64 + lane;
    for (int s = 0; s < nst; ++s) {
      const float* ws = wchunk + s * NT * 64;
      const float* as = As + lane_off + 4 * s + lk;
#pragma unroll
      for (int kz = 0; kz < 3; ++kz)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int tap = (kz * 3 + ky) * 3 + kx;
            float bf[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) bf[j] = ws[tap * tap_stride + j * 64];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
              if (m < mact) {
                const float af = as[((kz * MT_HY + ky) * MT_HX + 4 * m + kx) * MT_CKP];
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf[j], acc[m][j], 0, 0, 0);
              }
            }
          }
    }
  }

  // D: col = lane & 15 (cout), row = 4 (lane >> 4) + r = voxel (dy = lane >> 4, dx = r) of the M block
  if (mact == 0) return;
  const int oz = z0 + wz, oy = y0 + wy + lk;
  if (oy >= P.oh) return;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int co = 16 * j + li;
      if (co >= P.cout) continue;
      const float bias = P.bias ? P.bias[co] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ox = x0 + 4 * m + r;
        if (ox >= P.ow) continue;
        const long long vox = ((long long)oz * P.oh + oy) * P.ow + ox;
        float v = acc[m][j][r];
        if (P.bias) v += bias;
        P.out[img * P.out_istride + vox * P.out_ld + co] = mala_act(v, P.act);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------- wide
constexpr int MW_BM = 128, MW_KC = 16, MW_AP = 20, MW_BP = 80;

struct WideParams {
  const float* in; int in_ld; long long in_istride;
  int h, w;                    // input plane
  int od, oh, ow;              // GEMM rows: the output grid (valid conv) or the low-resolution grid (merge)
  int M, cin, cout, coutp, nck, nq, taps;
  const float* wp;             // [taps][cin][coutp]
  const float* bias;
  const float* dw;             // merge: transposed-conv weight [cin][9]
  const float* skip; int sk_ld; long long sk_istride; int sk_h, sk_w, crop_z, crop_xy;
  float* out; int out_ld; long long out_istride;
  float* ws; int split;        // split > 1: partial sums ws[split][M][coutp]
  int act, vec, n_base, ntn;   // vec: 16-byte A loads; n_base: first column of this launch; ntn: N tiles per sub-position
};

template <int NJ, bool MERGE>
__global__ __launch_bounds__(256) void conv3d_wide_kernel(WideParams P) {
  constexpr int BN = 16 * NJ, B4 = 4 * NJ;     // float4s per B row
  __shared__ __attribute__((aligned(16))) float As[2][MW_BM * MW_AP];
  __shared__ __attribute__((aligned(16))) float Bs[2][MW_KC * MW_BP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int m0 = blockIdx.x * MW_BM;
  const int sub = MERGE ? (int)blockIdx.y / P.ntn : 0;
  const int n0 = P.n_base + (MERGE ? (int)blockIdx.y % P.ntn : (int)blockIdx.y) * BN;
  const int kz_split = blockIdx.z;
  const int q0 = (int)((long long)P.nq * kz_split / P.split), q1 = (int)((long long)P.nq * (kz_split + 1) / P.split);

  // A staging: thread t fills 4 channels of rows t/4 and t/4 + 64
  const int c4 = (tid & 3) * 4;
  long long abase[2];
  bool arow[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int m = m0 + (tid >> 2) + 64 * u;
    arow[u] = m < P.M;
    int t = arow[u] ? m : 0;
    const int x = t % P.ow; t /= P.ow;
    const int y = t % P.oh; t /= P.oh;
    const int z = t % P.od;
    const int b = t / P.od;
    abase[u] = b * P.in_istride + (((long long)z * P.h + y) * P.w + x) * P.in_ld;
  }
  // B staging: thread t < 16 B4 fills 4 columns of row t / B4
  const bool bthr = tid < MW_KC * B4;
  const int brow = tid / B4, bcol = (tid % B4) * 4;

  float4 ra[2], rb;
  auto load = [&](int q) {
    const int tap = q / P.nck, cc0 = (q - tap * P.nck) * MW_KC;
    const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
    const long long toff = (((long long)kz * P.h + ky) * P.w + kx) * P.in_ld + cc0 + c4;
    const int cleft = P.cin - cc0 - c4;        // channels of this thread's group that exist
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (arow[u] && cleft > 0) {
        const float* src = P.in + abase[u] + toff;
        if (P.vec && cleft >= 4) v = *(const float4*)src;
        else {
          v.x = src[0];
          if (cleft > 1) v.y = src[1];
          if (cleft > 2) v.z = src[2];
          if (cleft > 3) v.w = src[3];
        }
        if (MERGE) {                             // dconv output = x[c] * wt[c][sub], one rounding as in the reference
          const float* d = P.dw + (long long)(cc0 + c4) * 9 + sub;
          v.x = v.x * d[0];
          if (cleft > 1) v.y = v.y * d[9];
          if (cleft > 2) v.z = v.z * d[18];
          if (cleft > 3) v.w = v.w * d[27];
        }
      }
      ra[u] = v;
    }
    rb = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bthr && cc0 + brow < P.cin) rb = *(const float4*)(P.wp + ((long long)tap * P.cin + cc0 + brow) * P.coutp + n0 + bcol);
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 2; ++u) *(float4*)&As[buf][((tid >> 2) + 64 * u) * MW_AP + c4] = ra[u];
    if (bthr) *(float4*)&Bs[buf][brow * MW_BP + bcol] = rb;
  };

  f32x4m acc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4m{0.f, 0.f, 0.f, 0.f};

  if (q0 < q1) {
    load(q0);
    store(0);
    __syncthreads();
  }
  for (int q = q0; q < q1; ++q) {
    const int buf = (q - q0) & 1;
    if (q + 1 < q1) load(q + 1);
    const int cc = min(MW_KC, P.cin - (q % P.nck) * MW_KC), nst = (cc + 3) >> 2;
    const float* a = &As[buf][(wave * 32 + li) * MW_AP + lk];
    const float* bb = &Bs[buf][lk * MW_BP + li];
    for (int s = 0; s < nst; ++s) {
      float af[2], bf[NJ];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = a[i * 16 * MW_AP + 4 * s];
#pragma unroll
      for (int j = 0; j < NJ; ++j) bf[j] = bb[4 * s * MW_BP + 16 * j];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (q + 1 < q1) store(buf ^ 1);
    __syncthreads();
  }

  // D: col = lane & 15 (cout), row = 4 (lane >> 4) + r (voxel)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wave * 32 + i * 16 + 4 * lk + r;
      if (m >= P.M) continue;
      if (P.split > 1) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int n = n0 + 16 * j + li;
          if (n < P.cout) P.ws[((long long)kz_split * P.M + m) * P.coutp + n] = acc[i][j][r];
        }
        continue;
      }
      int t = m;
      const int x = t % P.ow; t /= P.ow;
      const int y = t % P.oh; t /= P.oh;
      const int z = t % P.od;
      const int b = t / P.od;
      long long o, sk = 0;
      if (MERGE) {
        const int Y = 3 * y + sub / 3, X = 3 * x + sub % 3;
        o = b * P.out_istride + (((long long)z * 3 * P.oh + Y) * 3 * P.ow + X) * P.out_ld;
        sk = b * P.sk_istride + (((long long)(z + P.crop_z) * P.sk_h + Y + P.crop_xy) * P.sk_w + X + P.crop_xy) * P.sk_ld;
      } else {
        o = b * P.out_istride + (((long long)z * P.oh + y) * P.ow + x) * P.out_ld;
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int n = n0 + 16 * j + li;
        if (n >= P.cout) continue;
        float v = acc[i][j][r];
        if (P.bias) v += P.bias[n];
        if (MERGE) v += P.skip[sk + n];
        P.out[o + n] = mala_act(v, P.act);
      }
    }
}

// split-K: out = act(sum_s ws[s] + bias), s in order
__global__ void conv3d_wide_reduce_kernel(WideParams P) {
  const long long total = (long long)P.M * P.cout;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int m = (int)(e / P.cout), n = (int)(e - (long long)m * P.cout);
    float v = P.ws[(long long)m * P.coutp + n];
    for (int s = 1; s < P.split; ++s) v += P.ws[((long long)s * P.M + m) * P.coutp + n];
    if (P.bias) v += P.bias[n];
    int t = m;
    const int x = t % P.ow; t /= P.ow;
    const int y = t % P.oh; t /= P.oh;
    const int z = t % P.od;
    const int b = t / P.od;
    P.out[b * P.out_istride + (((long long)z * P.oh + y) * P.ow + x) * P.out_ld + n] = mala_act(v, P.act);
  }
}

static int mala_grid(long long total) {
  const long long b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 65536LL * 8 ? 65536LL * 8 : b));
}

// K split of a wide convolution: enough workgroups for the 256 CUs, at least 16 K chunks per split, at most 16 splits.  Chosen from ONE
// image's output voxels, so an image's result does not depend on the batch it runs in (the summation order is the same for every batch).
static int wide_split(long long M, int cout, int cin) {
  const long long tiles = ((M + MW_BM - 1) / MW_BM) * ((cout + 63) / 64);
  const int nq = 27 * ((cin + MW_KC - 1) / MW_KC);
  if (tiles >= 512) return 1;
  long long s = (1024 + tiles - 1) / tiles;
  s = s < nq / 16 ? s : nq / 16;
  s = s < 16 ? s : 16;
  return (int)(s < 1 ? 1 : s);
}

template <bool MERGE>
static void launch_wide(WideParams p, int subs, hipStream_t st) {
  const int full = p.cout / 64, rem = p.cout - full * 64, nj_tail = (rem + 15) / 16;    // 0..4
  const dim3 blk(256);
  p.ntn = full;
  p.n_base = 0;
  if (full > 0) conv3d_wide_kernel<4, MERGE><<<dim3((p.M + MW_BM - 1) / MW_BM, subs * full, p.split), blk, 0, st>>>(p);
  if (nj_tail == 0) return;
  p.ntn = 1;
  p.n_base = full * 64;
  const dim3 g((p.M + MW_BM - 1) / MW_BM, subs, p.split);
  switch (nj_tail) {
    case 1: conv3d_wide_kernel<1, MERGE><<<g, blk, 0, st>>>(p); break;
    case 2: conv3d_wide_kernel<2, MERGE><<<g, blk, 0, st>>>(p); break;
    case 3: conv3d_wide_kernel<3, MERGE><<<g, blk, 0, st>>>(p); break;
    default: conv3d_wide_kernel<4, MERGE><<<g, blk, 0, st>>>(p); break;     // cout < 64 with 49..63 columns
  }
}

// ------------------------------------------------------------------------------------------------------------------------------- misc
__global__ void maxpool133_kernel(const float* __restrict__ in, int in_ld, int nimg, int h, int w, int c, float* __restrict__ out, int out_ld) {
  const int ho = h / 3, wo = w / 3;
  const long long total = (long long)nimg * ho * wo * c;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % c);
    long long p = i / c;
    const int ox = (int)(p % wo); p /= wo;
    const int oy = (int)(p % ho);
    const long long n = p / ho;
    const float* src = in + ((n * h + 3 * oy) * w + 3 * ox) * in_ld + ch;
    float v = src[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const float t = src[((long long)dy * w + dx) * in_ld];
        v = (t > v || t != t) ? t : v;              // NaN propagates, as torch's max pool
      }
    out[((n * ho + oy) * wo + ox) * out_ld + ch] = v;
  }
}

// Provider_valid.add_vol for 'mala': out[c][z][y][x] = preds[k][c][z - oz][y - oy][x - ox] of the LAST window k that covers the voxel
__global__ void affinity_place_kernel(const float* __restrict__ preds, int nc, const int* __restrict__ org, int nw, int cz, int cy, int cx,
                                      float* __restrict__ out, int Z, int H, int W, int bz, int by, int bx, int bdz, int bdy, int bdx) {
  const long long total = (long long)bdz * bdy * bdx, vol = (long long)Z * H * W, per = (long long)cz * cy * cx;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i;
    const int x = bx + (int)(r % bdx); r /= bdx;
    const int y = by + (int)(r % bdy);
    const int z = bz + (int)(r / bdy);
    if (z >= Z || y >= H || x >= W) continue;
    for (int k = nw - 1; k >= 0; --k) {
      const int dz = z - org[3 * k], dy = y - org[3 * k + 1], dx = x - org[3 * k + 2];
      if ((unsigned)dz >= (unsigned)cz || (unsigned)dy >= (unsigned)cy || (unsigned)dx >= (unsigned)cx) continue;
      const long long l = ((long long)dz * cy + dy) * cx + dx, q = ((long long)z * H + y) * W + x;
      for (int c = 0; c < nc; ++c) out[c * vol + q] = preds[((long long)k * nc + c) * per + l];
      break;
    }
  }
}

}  // namespace gpemsr

using namespace gpemsr;
static_assert(sizeof(gpemsr_conv3d_valid_desc) == 112, "gpemsr_conv3d_valid_desc layout (gpemsr_amd/_abi.py Conv3dValidDesc)");

static int valid_common(const gpemsr_conv3d_valid_desc* d, const char* what) {
  GP_REQUIRE(d && d->in && d->weight && d->out, "%s: null pointer", what);
  GP_REQUIRE(d->n > 0 && d->d >= 3 && d->h >= 3 && d->w >= 3, "%s: input %dx%dx%d is smaller than the 3x3x3 kernel", what, d->d, d->h, d->w);
  GP_REQUIRE(d->cin > 0 && d->cout > 0 && d->in_ld >= d->cin && d->out_ld >= d->cout, "%s: channels / strides", what);
  GP_REQUIRE(d->act == GPEMSR_ACT_NONE || d->act == GPEMSR_ACT_LRELU_005 || d->act == GPEMSR_ACT_SIGMOID, "%s: act %d", what, d->act);
  return GPEMSR_OK;
}

extern "C" int gpemsr_conv3d_valid_thin(const gpemsr_conv3d_valid_desc* d, void* stream) {
  if (int rc = valid_common(d, "conv3d_valid_thin")) return rc;
  GP_REQUIRE(d->cout <= 80, "conv3d_valid_thin: cout %d > 80", d->cout);
  ThinParams p;
  p.in = d->in; p.in_ld = d->in_ld;
  p.in_istride = d->in_image_stride ? d->in_image_stride : (long long)d->d * d->h * d->w * d->in_ld;
  p.d = d->d; p.h = d->h; p.w = d->w; p.od = d->d - 2; p.oh = d->h - 2; p.ow = d->w - 2;
  p.cin = d->cin; p.cout = d->cout; p.ks4 = (d->cin + 3) / 4;
  p.wp = d->weight; p.bias = d->bias;
  p.out = d->out; p.out_ld = d->out_ld;
  p.out_istride = d->out_image_stride ? d->out_image_stride : (long long)p.od * p.oh * p.ow * d->out_ld;
  p.act = d->act;
  p.tiles_x = cdiv(p.ow, MT_TW); p.tiles_y = cdiv(p.oh, MT_TH); p.tiles_z = cdiv(p.od, MT_TZ);
  const long long blocks = (long long)p.tiles_x * p.tiles_y * p.tiles_z * d->n;
  GP_REQUIRE(blocks < (1LL << 31), "conv3d_valid_thin: grid too large");
  hipStream_t st = (hipStream_t)stream;
  switch ((d->cout + 15) / 16) {
    case 1: conv3d_valid_thin_kernel<1><<<(int)blocks, 256, 0, st>>>(p); break;
    case 2: conv3d_valid_thin_kernel<2><<<(int)blocks, 256, 0, st>>>(p); break;
    case 3: conv3d_valid_thin_kernel<3><<<(int)blocks, 256, 0, st>>>(p); break;
    case 4: conv3d_valid_thin_kernel<4><<<(int)blocks, 256, 0, st>>>(p); break;
    default: conv3d_valid_thin_kernel<5><<<(int)blocks, 256, 0, st>>>(p); break;
  }
  return check_launch("conv3d_valid_thin");
}

extern "C" int64_t gpemsr_conv3d_valid_thin_weight_floats(int cin, int cout) {
  if (cin <= 0 || cout <= 0 || cout > 80) return -1;
  return 27LL * ((cin + 3) / 4) * ((cout + 15) / 16) * 64;
}

extern "C" int64_t gpemsr_conv3d_valid_wide_weight_floats(int cin, int cout) {
  if (cin <= 0 || cout <= 0) return -1;
  return 27LL * cin * ((cout + 15) / 16 * 16);
}

extern "C" int64_t gpemsr_conv3d_valid_wide_workspace_floats(int n, int d, int h, int w, int cin, int cout) {
  if (n <= 0 || d < 3 || h < 3 || w < 3 || cin <= 0 || cout <= 0) return -1;
  const long long M = (long long)n * (d - 2) * (h - 2) * (w - 2);
  const int s = wide_split(M / n, cout, cin);
  return s > 1 ? s * M * ((cout + 15) / 16 * 16) : 0;
}

extern "C" int gpemsr_conv3d_valid_wide(const gpemsr_conv3d_valid_desc* d, void* stream) {
  if (int rc = valid_common(d, "conv3d_valid_wide")) return rc;
  WideParams p = {};
  p.in = d->in; p.in_ld = d->in_ld;
  p.in_istride = d->in_image_stride ? d->in_image_stride : (long long)d->d * d->h * d->w * d->in_ld;
  p.h = d->h; p.w = d->w; p.od = d->d - 2; p.oh = d->h - 2; p.ow = d->w - 2;
  const long long M = (long long)d->n * p.od * p.oh * p.ow;
  GP_REQUIRE(M < (1LL << 31) / 2, "conv3d_valid_wide: too many output voxels");
  p.M = (int)M; p.cin = d->cin; p.cout = d->cout; p.coutp = (d->cout + 15) / 16 * 16;
  p.nck = (d->cin + MW_KC - 1) / MW_KC; p.taps = 27; p.nq = 27 * p.nck;
  p.wp = d->weight; p.bias = d->bias;
  p.out = d->out; p.out_ld = d->out_ld;
  p.out_istride = d->out_image_stride ? d->out_image_stride : (long long)p.od * p.oh * p.ow * d->out_ld;
  p.act = d->act;
  p.vec = (d->in_ld % 4 == 0) && (d->cin % 4 == 0) && (((uintptr_t)d->in & 15) == 0) && (p.in_istride % 4 == 0);
  GP_REQUIRE(((uintptr_t)d->weight & 15) == 0, "conv3d_valid_wide: weight must be 16-byte aligned");
  p.split = wide_split(M / d->n, d->cout, d->cin);
  if (p.split > 1) {
    GP_REQUIRE(d->workspace && d->workspace_floats >= (long long)p.split * M * p.coutp,
               "conv3d_valid_wide: workspace of %lld floats needed", (long long)p.split * M * p.coutp);
    p.ws = d->workspace;
  }
  hipStream_t st = (hipStream_t)stream;
  launch_wide<false>(p, 1, st);
  if (p.split > 1) conv3d_wide_reduce_kernel<<<mala_grid(M * d->cout), 256, 0, st>>>(p);
  return check_launch("conv3d_valid_wide");
}

extern "C" int gpemsr_mala_merge(const float* x, int x_ld, int n, int d, int h, int w, int cin, const float* dw, const float* weight,
                                 const float* bias, int cout, const float* skip, int sk_ld, int sk_d, int sk_h, int sk_w, float* out, int out_ld,
                                 void* stream) {
  GP_REQUIRE(x && dw && weight && skip && out, "mala_merge: null pointer");
  GP_REQUIRE(n > 0 && d > 0 && h > 0 && w > 0 && cin > 0 && cout > 0 && x_ld >= cin && sk_ld >= cout && out_ld >= cout, "mala_merge: geometry");
  const int cz = (sk_d - d) / 2, c = (sk_h - 3 * h) / 2;
  GP_REQUIRE(cz > 0 && c > 0 && sk_d - 2 * cz == d && sk_h - 2 * c == 3 * h && sk_w - 2 * c == 3 * w,
             "mala_merge: skip %dx%dx%d does not crop to %dx%dx%d", sk_d, sk_h, sk_w, d, 3 * h, 3 * w);
  GP_REQUIRE(((uintptr_t)weight & 15) == 0, "mala_merge: weight must be 16-byte aligned");
  const long long M = (long long)n * d * h * w;
  GP_REQUIRE(M < (1LL << 31) / 2, "mala_merge: too many voxels");
  WideParams p = {};
  p.in = x; p.in_ld = x_ld; p.in_istride = (long long)d * h * w * x_ld;
  p.h = h; p.w = w; p.od = d; p.oh = h; p.ow = w;
  p.M = (int)M; p.cin = cin; p.cout = cout; p.coutp = (cout + 15) / 16 * 16;
  p.nck = (cin + MW_KC - 1) / MW_KC; p.taps = 1; p.nq = p.nck;
  p.wp = weight; p.bias = bias; p.dw = dw;
  p.skip = skip; p.sk_ld = sk_ld; p.sk_istride = (long long)sk_d * sk_h * sk_w * sk_ld; p.sk_h = sk_h; p.sk_w = sk_w;
  p.crop_z = cz; p.crop_xy = c;
  p.out = out; p.out_ld = out_ld; p.out_istride = (long long)d * 9 * h * w * out_ld;
  p.split = 1; p.act = GPEMSR_ACT_NONE;
  p.vec = (x_ld % 4 == 0) && (cin % 4 == 0) && (((uintptr_t)x & 15) == 0);
  launch_wide<true>(p, 9, (hipStream_t)stream);
  return check_launch("mala_merge");
}

extern "C" int gpemsr_maxpool133(const float* in, int in_ld, int nimg, int h, int w, int c, float* out, int out_ld, void* stream) {
  GP_REQUIRE(in && out, "maxpool133: null pointer");
  GP_REQUIRE(nimg > 0 && h >= 3 && w >= 3 && c > 0 && in_ld >= c && out_ld >= c, "maxpool133: geometry");
  maxpool133_kernel<<<mala_grid((long long)nimg * (h / 3) * (w / 3) * c), 256, 0, (hipStream_t)stream>>>(in, in_ld, nimg, h, w, c, out, out_ld);
  return check_launch("maxpool133");
}

extern "C" int gpemsr_affinity_place(const float* preds, int nc, const int32_t* origins, int nw, int cz, int cy, int cx, float* out, int Z, int H,
                                     int W, const int32_t* bbox, void* stream) {
  GP_REQUIRE(preds && origins && out && bbox && nw > 0 && nc >= 1, "affinity_place: null pointer / no windows");
  GP_REQUIRE(Z > 0 && H > 0 && W > 0 && cz > 0 && cy > 0 && cx > 0, "affinity_place: geometry");
  GP_REQUIRE(bbox[0] >= 0 && bbox[1] >= 0 && bbox[2] >= 0 && bbox[3] > 0 && bbox[4] > 0 && bbox[5] > 0, "affinity_place: bbox");
  const long long total = (long long)bbox[3] * bbox[4] * bbox[5];
  affinity_place_kernel<<<mala_grid(total), 256, 0, (hipStream_t)stream>>>(preds, nc, origins, nw, cz, cy, cx, out, Z, H, W, bbox[0], bbox[1],
                                                                           bbox[2], bbox[3], bbox[4], bbox[5]);
  return check_launch("affinity_place");
}
