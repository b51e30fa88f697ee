// The affinity U-Net of the segmentation step (gpemsr_amd/affinity.py): 3-D convolution on the f32 matrix pipe, the upsample/merge
// prologue of its decoder, and the volume kernels of the sliding-window inference (window gather, Gaussian-weighted stitching, divide + crop).
//
// gpemsr_conv3d -- implicit GEMM, D[voxel][cout] = sum_{tap} sum_{cin} In[voxel + tap][cin] * W[tap][cin][cout], on v_mfma_f32_16x16x4_f32
// (exact f32: one rounding per product, guide section 3).  16x16x4 rather than 32x32x2 because of the network's channel counts: cout is padded
// to a multiple of 16 (28 -> 32, 36 -> 48, 48 / 64 / 80 exact) instead of 32 (36 -> 64 wastes 44 %), and cin only to a multiple of 4 (all
// five widths are), so the executed / algorithmic FLOP ratio of the 3x3x3 layers is 1.14 (28), 1.33 (36) and 1.00 (48, 64, 80).
//
//   workgroup  = 4 waves, output tile TZ x TH x TW = 2 x 8 x 16 voxels x every cout (NT = cout_pad / 16 tiles of 16)
//   wave w     = output slice z0 + w / 2, rows y0 + 4 (w % 2) .. + 3: four 16-voxel M tiles, 4 x NT accumulators (<= 80 VGPRs)
//   K loop     = cin chunks of 16 channels; per chunk the (TZ + KD - 1) x (TH + KS - 1) x (TW + KS - 1) input halo is staged ONCE in LDS
//                (zero padding = zero fill) and every one of the KD * KS * KS taps reads it at a shifted offset: 27-fold reuse for 3x3x3, and
//                the halo of a 2-slice tile reads 4 input slices (2x, not the 3x of a slice-per-tile form)
//   A operand  = LDS, one float per lane: lane (i = lane & 15, k = lane >> 4) holds voxel i's channel 4 s + k.  Voxels are 18 floats apart
//                (16 channels + 2 pad): the 32 lanes of a ds_read_b32 group hit 32 distinct banks
//   B operand  = the packed weights straight from global memory (L1 / L2 resident: <= 691 KB per layer): lane l reads float l of a 256-B
//                fragment [k = l >> 4][n = l & 15], coalesced; per k-step a wave issues NT such loads for 4 * NT MFMAs
//   epilogue   = (+ bias) (+ residual) (* scale + shift: a folded eval-mode BatchNorm) (ELU | sigmoid), stored at out + voxel * out_ld + c *
//                out_cstride, so the same kernel writes NDHWC activations and the NCDHW [B, 3, D, H, W] affinities.
// LDS: 51.8 KB for 3x3x3 (720 halo voxels), 34.6 KB for 1x5x5, 18.4 KB for 1x1x1: three workgroups per CU.
//
// The stitching kernels reproduce Provider_valid.add_vol / get_results (data/provider_valid.py:270-298) BIT FOR BIT: one thread per voxel walks
// the windows that cover it in index order, out = out + a * w and wmap = wmap + w as separately rounded f32 operations (no atomics; FMA
// contraction switched off by pragma), then out / wmap.
#include "common.h"

namespace gpemsr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int C3_TW = 16, C3_TH = 8, C3_TZ = 2, C3_CK = 16, C3_CKP = 18, C3_NTMAX = 5;

struct Conv3dParams {
  const float* in; int in_ld; long long in_istride;
  int d, h, w, cin, cout, ks4;
  const float* wp;
  const float* bias; const float* scale; const float* shift;
  const float* res; int res_ld; long long res_istride;
  float* out; int out_ld; long long out_cs, out_istride;
  int act;
  int tiles_x, tiles_y, tiles_z;
};

__device__ __forceinline__ float act3(float v, int act) {
  if (act == GPEMSR_ACT_ELU) return v > 0.f ? v : expm1f(v);
  return apply_act(v, act);
}

template <int KD, int KS, int NT>
__global__ __launch_bounds__(256, 2) void conv3d_mfma_kernel(Conv3dParams P) {
  constexpr int HZ = C3_TZ + KD - 1, HY = C3_TH + KS - 1, HX = C3_TW + KS - 1, HVOX = HZ * HY * HX;
  __shared__ float As[HVOX * C3_CKP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int b = blockIdx.x;
  const int tx = b % P.tiles_x; b /= P.tiles_x;
  const int ty = b % P.tiles_y; b /= P.tiles_y;
  const int tz = b % P.tiles_z;
  const int img = b / P.tiles_z;
  const int x0 = tx * C3_TW, y0 = ty * C3_TH, z0 = tz * C3_TZ;
  const float* in = P.in + img * P.in_istride;
  const int wz = wave >> 1, wy = (wave & 1) * 4, li = lane & 15, lk = lane >> 4;

  f32x4 acc[4][NT];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long long tap_stride = (long long)P.ks4 * NT * 64;
  for (int c0 = 0; c0 < P.cin; c0 += C3_CK) {
    const int cc = min(C3_CK, P.cin - c0);
    const int nst = (cc + 3) >> 2, cc4 = nst * 4;
    __syncthreads();                                   // the previous chunk's fragment reads are done
    for (int e = tid; e < HVOX * cc4; e += 256) {
      const int v = e / cc4, c = e - v * cc4;
      const int hx = v % HX, t = v / HX, hy = t % HY, hz = t / HY;
      const int gz = z0 + hz - KD / 2, gy = y0 + hy - KS / 2, gx = x0 + hx - KS / 2;
      float val = 0.f;
      if (c < cc && (unsigned)gz < (unsigned)P.d && (unsigned)gy < (unsigned)P.h && (unsigned)gx < (unsigned)P.w)
        val = in[(((long long)gz * P.h + gy) * P.w + gx) * P.in_ld + c0 + c];
      As[v * C3_CKP + c] = val;
    }
    __syncthreads();
    const float* wchunk = P.wp + (long long)(c0 >> 2) * NT * 64 + lane;
    for (int s = 0; s < nst; ++s) {
      const float* ws = wchunk + s * NT * 64;
      const float* as = As + (wz * HY + wy) * HX * C3_CKP + li * C3_CKP + 4 * s + lk;
#pragma unroll
      for (int kz = 0; kz < KD; ++kz)
#pragma unroll
        for (int ky = 0; ky < KS; ++ky)
#pragma unroll
          for (int kx = 0; kx < KS; ++kx) {
            const int tap = (kz * KS + ky) * KS + kx;
            float bf[NT], af[4];
#pragma unroll
            for (int j = 0; j < NT; ++j) bf[j] = ws[tap * tap_stride + j * 64];
#pragma unroll
            for (int m = 0; m < 4; ++m) af[m] = as[((kz * HY + m + ky) * HX + kx) * C3_CKP];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
              for (int j = 0; j < NT; ++j) acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[m], bf[j], acc[m][j], 0, 0, 0);
          }
    }
  }

  // D: col = lane & 15 (cout within the tile), row = 4 (lane >> 4) + r (voxel x within the 16-voxel row)
  const int oz = z0 + wz;
  if (oz >= P.d) return;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int oy = y0 + wy + m;
    if (oy >= P.h) continue;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int co = 16 * j + li;
      if (co >= P.cout) continue;
      const float bias = P.bias ? P.bias[co] : 0.f;
      const float sc = P.scale ? P.scale[co] : 1.f, sh = P.scale ? P.shift[co] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ox = x0 + 4 * lk + r;
        if (ox >= P.w) continue;
        const long long vox = ((long long)oz * P.h + oy) * P.w + ox;
        float v = acc[m][j][r];
        if (P.bias) v += bias;
        if (P.res) v += P.res[img * P.res_istride + vox * P.res_ld + co];
        if (P.scale) v = v * sc + sh;
        P.out[img * P.out_istride + vox * P.out_ld + co * P.out_cs] = act3(v, P.act);
      }
    }
  }
}

template <int KD, int KS>
static void launch_conv3d(const Conv3dParams& p, int nt, int blocks, hipStream_t st) {
  switch (nt) {
    case 1: conv3d_mfma_kernel<KD, KS, 1><<<blocks, 256, 0, st>>>(p); break;
    case 2: conv3d_mfma_kernel<KD, KS, 2><<<blocks, 256, 0, st>>>(p); break;
    case 3: conv3d_mfma_kernel<KD, KS, 3><<<blocks, 256, 0, st>>>(p); break;
    case 4: conv3d_mfma_kernel<KD, KS, 4><<<blocks, 256, 0, st>>>(p); break;
    default: conv3d_mfma_kernel<KD, KS, 5><<<blocks, 256, 0, st>>>(p); break;
  }
}

// ---- up_k + cat_k of the decoder: ELU(scale * (bilinear2x_align_corners(low) + skip) + shift) ----
__global__ void upsample2_add_bn_elu_kernel(const float* __restrict__ low, int lo_ld, const float* __restrict__ skip, int sk_ld, int nimg, int h,
                                            int w, int c, const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ out,
                                            int out_ld) {
  const int H = 2 * h, W = 2 * w;
  const long long total = (long long)nimg * H * W * c;
  const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % c);
    long long p = i / c;
    const int ox = (int)(p % W); p /= W;
    const int oy = (int)(p % H);
    const long long n = p / H;
    const float fy = sy * oy, fx = sx * ox;
    const int iy0 = min((int)fy, h - 1), ix0 = min((int)fx, w - 1);
    const int iy1 = iy0 + (iy0 < h - 1), ix1 = ix0 + (ix0 < w - 1);
    const float ly = fy - iy0, lx = fx - ix0;
    const float* L = low + n * h * w * lo_ld + ch;
    const float v00 = L[((long long)iy0 * w + ix0) * lo_ld], v01 = L[((long long)iy0 * w + ix1) * lo_ld];
    const float v10 = L[((long long)iy1 * w + ix0) * lo_ld], v11 = L[((long long)iy1 * w + ix1) * lo_ld];
    const float up = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
    const long long q = (n * H + oy) * W + ox;
    const float v = (up + skip[q * sk_ld + ch]) * scale[ch] + shift[ch];
    out[q * out_ld + ch] = v > 0.f ? v : expm1f(v);
  }
}

__device__ __forceinline__ int reflect_index(int p, int n) {   // numpy.pad(mode='reflect') for a pad smaller than n
  if (p < 0) p = -p;
  if (p >= n) p = 2 * (n - 1) - p;
  return min(max(p, 0), n - 1);                                // (origins outside the padded volume read its edge, never out of bounds)
}

template <typename T>
__global__ void affinity_gather_kernel(const T* __restrict__ vol, int Z, int H, int W, int pz, int py, int px, const int* __restrict__ org,
                                       int nw, int cz, int cy, int cx, float* __restrict__ out) {
  const long long per = (long long)cz * cy * cx, total = per * nw;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i / per);
    long long r = i - k * per;
    const int dx = (int)(r % cx); r /= cx;
    const int dy = (int)(r % cy);
    const int dz = (int)(r / cy);
    const int z = reflect_index(org[3 * k] + dz - pz, Z), y = reflect_index(org[3 * k + 1] + dy - py, H),
              x = reflect_index(org[3 * k + 2] + dx - px, W);
    const T v = vol[((long long)z * H + y) * W + x];
    if constexpr (sizeof(T) == 1) out[i] = __fdiv_rn((float)v, 255.0f);   // astype(float32) / 255.0, a division as the reference's
    else out[i] = (float)v;
  }
}

// windows [k0, k0 + nw) of the plan, in index order; the thread grid covers their bounding box [bz, +bdz) x [by, +bdy) x [bx, +bdx)
__global__ void affinity_accumulate_kernel(const float* __restrict__ affs, int nc, const float* __restrict__ wvol, const int* __restrict__ org,
                                           int nw, int cz, int cy, int cx, float* __restrict__ out, float* __restrict__ wmap, int Zp, int Hp, int Wp,
                                           int bz, int by, int bx, int bdz, int bdy, int bdx) {
  // no FMA contraction in this body: hipcc's default -ffp-contract=fast-honor-pragmas fuses a * w + o into v_fmac_f32 (one rounding
  // instead of numpy's two) -- and it does so through __fmul_rn / __fadd_rn too, whose bodies live outside this pragma's scope
#pragma clang fp contract(off)
  const long long total = (long long)bdz * bdy * bdx, vol = (long long)Zp * Hp * Wp, per = (long long)cz * cy * cx;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i;
    const int x = bx + (int)(r % bdx); r /= bdx;
    const int y = by + (int)(r % bdy);
    const int z = bz + (int)(r / bdy);
    if (z >= Zp || y >= Hp || x >= Wp) continue;
    const long long q = ((long long)z * Hp + y) * Wp + x;
    float o[4], ws = 0.f;
    bool hit = false;
    for (int k = 0; k < nw; ++k) {
      const int dz = z - org[3 * k], dy = y - org[3 * k + 1], dx = x - org[3 * k + 2];
      if ((unsigned)dz >= (unsigned)cz || (unsigned)dy >= (unsigned)cy || (unsigned)dx >= (unsigned)cx) continue;
      if (!hit) {
        hit = true;
        ws = wmap[q];
        for (int c = 0; c < nc; ++c) o[c] = out[c * vol + q];
      }
      const long long l = ((long long)dz * cy + dy) * cx + dx;
      const float w = wvol[l];
      for (int c = 0; c < nc; ++c) {
        const float p = affs[((long long)k * nc + c) * per + l] * w;     // rounded on its own, then added (numpy's out += affs * w)
        o[c] = o[c] + p;
      }
      ws = ws + w;
    }
    if (hit) {
      wmap[q] = ws;
      for (int c = 0; c < nc; ++c) out[c * vol + q] = o[c];
    }
  }
}

__global__ void affinity_finalize_kernel(const float* __restrict__ out, const float* __restrict__ wmap, int nc, int Zp, int Hp, int Wp, int pz,
                                         int py, int px, int Z, int H, int W, float* __restrict__ res) {
  const long long total = (long long)nc * Z * H * W, vol = (long long)Zp * Hp * Wp;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i;
    const int x = (int)(r % W); r /= W;
    const int y = (int)(r % H); r /= H;
    const int z = (int)(r % Z);
    const int c = (int)(r / Z);
    const long long q = ((long long)(z + pz) * Hp + (y + py)) * Wp + (x + px);
    res[i] = __fdiv_rn(out[c * vol + q], wmap[q]);
  }
}

static int grid_for(long long total) {
  const long long b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 65536LL * 8 ? 65536LL * 8 : b));
}

}  // namespace gpemsr

using namespace gpemsr;
static_assert(sizeof(gpemsr_conv3d_desc) == 152, "gpemsr_conv3d_desc layout (gpemsr_amd/_abi.py Conv3dDesc)");

extern "C" int gpemsr_conv3d(const gpemsr_conv3d_desc* d, void* stream) {
  GP_REQUIRE(d && d->in && d->weight && d->out, "conv3d: null pointer");
  GP_REQUIRE(d->n > 0 && d->d > 0 && d->h > 0 && d->w > 0, "conv3d: empty geometry");
  GP_REQUIRE(d->cin > 0 && d->cout > 0 && d->cout <= 16 * C3_NTMAX, "conv3d: cout %d outside 1..%d", d->cout, 16 * C3_NTMAX);
  GP_REQUIRE(d->in_ld >= d->cin && d->out_ld >= 1 && d->out_cstride >= 1, "conv3d: strides");
  GP_REQUIRE(!d->residual || d->res_ld >= d->cout, "conv3d: residual ld");
  GP_REQUIRE(!d->scale == !d->shift, "conv3d: scale and shift go together");
  GP_REQUIRE(d->act == GPEMSR_ACT_NONE || d->act == GPEMSR_ACT_ELU || d->act == GPEMSR_ACT_SIGMOID, "conv3d: act %d", d->act);
  const bool shape_ok = (d->kd == 3 && d->ks == 3) || (d->kd == 1 && (d->ks == 1 || d->ks == 3 || d->ks == 5));
  GP_REQUIRE(shape_ok, "conv3d: kernel %dx%dx%d not built (3x3x3, 1x3x3, 1x5x5, 1x1x1)", d->kd, d->ks, d->ks);
  Conv3dParams p;
  p.in = d->in; p.in_ld = d->in_ld;
  p.in_istride = d->in_image_stride ? d->in_image_stride : (long long)d->d * d->h * d->w * d->in_ld;
  p.d = d->d; p.h = d->h; p.w = d->w; p.cin = d->cin; p.cout = d->cout; p.ks4 = (d->cin + 3) / 4;
  p.wp = d->weight; p.bias = d->bias; p.scale = d->scale; p.shift = d->shift;
  p.res = d->residual; p.res_ld = d->res_ld;
  p.res_istride = d->res_image_stride ? d->res_image_stride : (long long)d->d * d->h * d->w * d->res_ld;
  p.out = d->out; p.out_ld = d->out_ld; p.out_cs = d->out_cstride;
  p.out_istride = d->out_image_stride ? d->out_image_stride : (long long)d->d * d->h * d->w * d->out_ld;
  p.act = d->act;
  p.tiles_x = cdiv(d->w, C3_TW); p.tiles_y = cdiv(d->h, C3_TH); p.tiles_z = cdiv(d->d, C3_TZ);
  const long long blocks = (long long)p.tiles_x * p.tiles_y * p.tiles_z * d->n;
  GP_REQUIRE(blocks < (1LL << 31), "conv3d: grid too large");
  const int nt = (d->cout + 15) / 16;
  hipStream_t st = (hipStream_t)stream;
  if (d->kd == 3) launch_conv3d<3, 3>(p, nt, (int)blocks, st);
  else if (d->ks == 1) launch_conv3d<1, 1>(p, nt, (int)blocks, st);
  else if (d->ks == 3) launch_conv3d<1, 3>(p, nt, (int)blocks, st);
  else launch_conv3d<1, 5>(p, nt, (int)blocks, st);
  return check_launch("conv3d");
}

extern "C" int gpemsr_conv3d_weight_floats(int cin, int cout, int kd, int ks) {
  if (cin <= 0 || cout <= 0 || cout > 16 * C3_NTMAX) return -1;
  return kd * ks * ks * ((cin + 3) / 4) * ((cout + 15) / 16) * 64;
}

extern "C" int gpemsr_upsample2_add_bn_elu(const float* low, int lo_ld, const float* skip, int sk_ld, int nimg, int h, int w, int c,
                                           const float* scale, const float* shift, float* out, int out_ld, void* stream) {
  GP_REQUIRE(low && skip && scale && shift && out, "upsample2_add_bn_elu: null pointer");
  GP_REQUIRE(nimg > 0 && h > 0 && w > 0 && c > 0 && lo_ld >= c && sk_ld >= c && out_ld >= c, "upsample2_add_bn_elu: geometry");
  upsample2_add_bn_elu_kernel<<<grid_for((long long)nimg * 4 * h * w * c), 256, 0, (hipStream_t)stream>>>(low, lo_ld, skip, sk_ld, nimg, h, w, c,
                                                                                                           scale, shift, out, out_ld);
  return check_launch("upsample2_add_bn_elu");
}

extern "C" int gpemsr_affinity_gather(const void* vol, int is_u8, int Z, int H, int W, int pz, int py, int px, const int32_t* origins, int nw,
                                      int cz, int cy, int cx, float* out, void* stream) {
  GP_REQUIRE(vol && origins && out && nw > 0, "affinity_gather: null pointer / no windows");
  GP_REQUIRE(Z > 0 && H > 0 && W > 0 && cz > 0 && cy > 0 && cx > 0, "affinity_gather: geometry");
  GP_REQUIRE(pz >= 0 && py >= 0 && px >= 0 && pz < Z && py < H && px < W, "affinity_gather: reflect padding must be smaller than the extent");
  const long long total = (long long)nw * cz * cy * cx;
  if (is_u8)
    affinity_gather_kernel<uint8_t><<<grid_for(total), 256, 0, (hipStream_t)stream>>>((const uint8_t*)vol, Z, H, W, pz, py, px, origins, nw, cz, cy, cx, out);
  else
    affinity_gather_kernel<float><<<grid_for(total), 256, 0, (hipStream_t)stream>>>((const float*)vol, Z, H, W, pz, py, px, origins, nw, cz, cy, cx, out);
  return check_launch("affinity_gather");
}

extern "C" int gpemsr_affinity_accumulate(const float* affs, int nc, const float* wvol, const int32_t* origins, int nw, int cz, int cy, int cx,
                                          float* out, float* wmap, int Zp, int Hp, int Wp, const int32_t* bbox, void* stream) {
  GP_REQUIRE(affs && wvol && origins && out && wmap && bbox && nw > 0, "affinity_accumulate: null pointer / no windows");
  GP_REQUIRE(nc >= 1 && nc <= 4, "affinity_accumulate: %d channels (1..4)", nc);
  GP_REQUIRE(bbox[0] >= 0 && bbox[1] >= 0 && bbox[2] >= 0 && bbox[3] > 0 && bbox[4] > 0 && bbox[5] > 0, "affinity_accumulate: bbox");
  const long long total = (long long)bbox[3] * bbox[4] * bbox[5];
  affinity_accumulate_kernel<<<grid_for(total), 256, 0, (hipStream_t)stream>>>(affs, nc, wvol, origins, nw, cz, cy, cx, out, wmap, Zp, Hp, Wp,
                                                                              bbox[0], bbox[1], bbox[2], bbox[3], bbox[4], bbox[5]);
  return check_launch("affinity_accumulate");
}

extern "C" int gpemsr_affinity_finalize(const float* out, const float* wmap, int nc, int Zp, int Hp, int Wp, int pz, int py, int px, int Z, int H,
                                        int W, float* res, void* stream) {
  GP_REQUIRE(out && wmap && res && nc >= 1, "affinity_finalize: null pointer");
  GP_REQUIRE(Z > 0 && H > 0 && W > 0 && pz >= 0 && py >= 0 && px >= 0 && Z + 2 * pz <= Zp && H + 2 * py <= Hp && W + 2 * px <= Wp,
             "affinity_finalize: crop outside the padded volume");
  affinity_finalize_kernel<<<grid_for((long long)nc * Z * H * W), 256, 0, (hipStream_t)stream>>>(out, wmap, nc, Zp, Hp, Wp, pz, py, px, Z, H, W, res);
  return check_launch("affinity_finalize");
}
