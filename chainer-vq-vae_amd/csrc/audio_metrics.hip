// Objective audio metrics over a ragged list of waveforms (include/vqvae_metrics.h): STFT -> power -> mel -> log in one
// launch per chunk, and the three per-utterance distances in one more.
//
// metrics_stft_mel_kernel: a workgroup of four waves owns a tile of 32 frames (plain frames of the ragged frame axis: a tile
//   may span several utterances and an utterance many tiles; a thread per frame finds the frame's utterance once by a
//   search in the frame_off prefix table and leaves the frame's first sample in LDS).
//   The DFT is a GEMM on the matrix pipe, dft (2 nb x n_fft) against the frame matrix (n_fft x 32), the im2col of the wave,
//   which is never written to memory.  Two ways to a frame's samples, chosen per tile, the arithmetic the same in both:
//     staged  the tile lies inside ONE utterance and its n_fft + (frames - 1) * hop contiguous samples fit in LDS beside the
//             power spectrum: they are staged once, every frame reads its own window from there.  Sample s is kept at
//             s + (s >> 5) + (s >> 10): the 32 lanes of an operand read are hop samples apart, which for a hop that is a
//             multiple of 32 would be ONE bank; with the skew they are 32 banks for every power-of-two hop.
//     direct  a tile that spans utterances (or a window too long to stage): every lane reads its frame's samples from global
//             memory (L1 / L2 hold them: a window is read by every row tile).
//   A wave owns the row tiles wave, wave + 4, ...: 32 bins, the re and the im accumulator of the SAME bins, so the power is
//   formed in registers.  The A operand comes straight from the table in global memory: lane (row lr, half lh) loads the 8
//   contiguous floats dft[row][k0 + 8 lh ..] of a block of 16 samples (two 16-byte loads per accumulator; the next block's
//   travel while the matrix pipe works on this one's), and MFMA step j of the block takes k0 + j from the lower half-wave
//   and k0 + 8 + j from the upper -- that fixes the K order of the header.  nb is odd: the last row tile holds the Nyquist bin
//   alone beside rows that do not exist; those are neither loaded (exec-masked loads, zeros as operands) nor stored.
//   The power of the tile goes to LDS ([bin][frame]: conflict-free both ways), mag is stored from the accumulators, and after
//   one barrier thread (frame, mel row mod 8) adds its mel rows over the bins in ascending order (one LDS read serves four
//   mel rows) and stores logf(max(., floor)) (and the sum itself, when asked for).  Frames past ftot repeat the last valid frame's samples and are never stored.
//   LDS (dynamic): 384 + 128 nb bytes, + 4 (skew(n_fft + 31 hop - 1) + 1) when staged: 103 KB at the default configuration
//   (n_fft 1024, hop 256), opted in once; one workgroup per CU, whose four waves keep two independent accumulators each.
// metrics_distances_kernel: one workgroup of 256 threads per utterance pair; float64 in the fixed order of the header,
//   no atomics; compiled without contraction (-ffp-contract=off, the Makefile's setting for the whole library).
//
// Every address is formed in 64 bits.  Stores: log_mel[m * stride + f] (and mel_pw) for m < n_mels, mag[b * stride + f] for b < nb, both for
// f < ftot only; out[3 i + 0 .. 2]; plain vector stores.
#include "common.h"
#include "ragged_seg.h"
#include "../../include/vqvae_metrics.h"

namespace vq {

using mt_f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int MT_TILE = VQVAE_METRICS_TILE;
constexpr int MT_THREADS = VQVAE_METRICS_THREADS;
constexpr size_t MT_LDS_CAP = 160 * 1024;          // the LDS of a CU, which one workgroup may take

struct StftArgs {
  const float* x; const int64_t* off_in; const int64_t* frame_off; const float* dft; const float* mel;
  float* log_mel; float* mag; float* mel_pw;
  long long ftot, stride;
  int n, n_fft, hop, n_mels, nb, stage_ok;
  float floor;
};

// where sample s of a staged tile is kept (see above); monotonic, so the image of [0, len) ends at mt_skew(len - 1)
__host__ __device__ __forceinline__ int mt_skew(int s) { return s + (s >> 5) + (s >> 10); }

static size_t mt_lds_direct(int nb) { return (size_t)MT_TILE * (sizeof(long long) + sizeof(int)) + (size_t)nb * MT_TILE * sizeof(float); }
static size_t mt_lds_staged(int n_fft, int hop, int nb) {
  return mt_lds_direct(nb) + ((size_t)mt_skew(n_fft + (MT_TILE - 1) * hop - 1) + 1) * sizeof(float);
}

__global__ __launch_bounds__(MT_THREADS) void metrics_stft_mel_kernel(StftArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mt_lds[];
  long long* s_g = reinterpret_cast<long long*>(mt_lds);       // [32] first sample of the frame in x
  int* s_utt = reinterpret_cast<int*>(s_g + MT_TILE);          // [32] its utterance
  float* s_pw = reinterpret_cast<float*>(s_utt + MT_TILE);     // [nb][32] power
  float* s_x = s_pw + (size_t)a.nb * MT_TILE;                  // staged samples, skewed

  const int tid = threadIdx.x;
  const long long f0 = (long long)blockIdx.x * MT_TILE;
  const long long left = a.ftot - f0;
  const int nv = left < MT_TILE ? (int)left : MT_TILE;         // frames of this tile, >= 1
  if (tid < MT_TILE) {
    const long long f = f0 + (tid < nv ? tid : nv - 1);        // a column past the end repeats the last frame: computed, never stored
    const int i = ragged_find_segment(a.frame_off, a.n, f);      // the utterance of frame f
    s_g[tid] = (long long)a.off_in[i] + (f - (long long)a.frame_off[i]) * a.hop;
    s_utt[tid] = i;
  }
  __syncthreads();
  const bool staged = a.stage_ok && s_utt[0] == s_utt[nv - 1];     // the same for the whole workgroup
  if (staged) {
    const int len = a.n_fft + (nv - 1) * a.hop;                // exactly the samples the tile's frames cover
    const float* src = a.x + s_g[0];
    for (int s = tid; s < len; s += MT_THREADS) s_x[mt_skew(s)] = src[s];
    __syncthreads();
  }

  const int wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 31, lh = lane >> 5;
  const int col = lr < nv ? lr : nv - 1;
  const int nbt = (a.nb + 31) >> 5;

  auto row_tiles = [&](auto sample) {
    for (int bt = wave; bt < nbt; bt += 4) {
      const int row = bt * 32 + lr;
      const bool rok = row < a.nb;
      const float4* pre = reinterpret_cast<const float4*>(a.dft + (long long)(rok ? row : 0) * a.n_fft + 8 * lh);
      const float4* pim = reinterpret_cast<const float4*>(a.dft + (long long)(a.nb + (rok ? row : 0)) * a.n_fft + 8 * lh);
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      float4 cr0 = z, cr1 = z, ci0 = z, ci1 = z, nr0 = z, nr1 = z, ni0 = z, ni1 = z;
      if (rok) { cr0 = pre[0]; cr1 = pre[1]; ci0 = pim[0]; ci1 = pim[1]; }
      mt_f32x16 are, aim;
#pragma unroll
      for (int r = 0; r < 16; ++r) { are[r] = 0.f; aim[r] = 0.f; }
      for (int k0 = 0; k0 < a.n_fft; k0 += 16) {
        if (rok && k0 + 16 < a.n_fft) {
          const int q = (k0 + 16) >> 2;
          nr0 = pre[q]; nr1 = pre[q + 1]; ni0 = pim[q]; ni1 = pim[q + 1];
        }
        const float ar[8] = {cr0.x, cr0.y, cr0.z, cr0.w, cr1.x, cr1.y, cr1.z, cr1.w};
        const float ai[8] = {ci0.x, ci0.y, ci0.z, ci0.w, ci1.x, ci1.y, ci1.z, ci1.w};
        float bv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) bv[j] = sample(k0 + 8 * lh + j);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          are = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[j], bv[j], are, 0, 0, 0);
          aim = __builtin_amdgcn_mfma_f32_32x32x2f32(ai[j], bv[j], aim, 0, 0, 0);
        }
        cr0 = nr0; cr1 = nr1; ci0 = ni0; ci1 = ni1;
      }
      // C/D layout of the 32 x 32 tiles: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int b = bt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (b < a.nb) {
          const float pw = are[r] * are[r] + aim[r] * aim[r];
          s_pw[b * MT_TILE + lr] = pw;
          if (a.mag && lr < nv) a.mag[(long long)b * a.stride + f0 + lr] = sqrtf(pw);
        }
      }
    }
  };
  if (staged) {
    const int sb = col * a.hop;
    row_tiles([&](const int k) { return s_x[mt_skew(sb + k)]; });
  } else {
    const float* xs = a.x + s_g[col];
    row_tiles([&](const int k) { return xs[k]; });
  }
  if (!a.log_mel && !a.mel_pw) return;
  __syncthreads();

  // mel[m] = sum_b mel[m, b] * pw[b], bins ascending; thread (frame fr, rows mr, mr + 8, mr + 16, mr + 24 of a group of 32)
  const int fr = tid & 31, mr = tid >> 5;
  for (int m0 = 0; m0 < a.n_mels; m0 += 32) {
    const float* wrow[4];
    float acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + mr + 8 * q;
      wrow[q] = a.mel + (long long)(m < a.n_mels ? m : a.n_mels - 1) * a.nb;     // a row past the end repeats the last: never stored
      acc[q] = 0.f;
    }
    for (int b = 0; b < a.nb; ++b) {
      const float p = s_pw[b * MT_TILE + fr];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] += wrow[q][b] * p;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + mr + 8 * q;
      if (m < a.n_mels && fr < nv) {
        const long long at = (long long)m * a.stride + f0 + fr;
        if (a.mel_pw) a.mel_pw[at] = acc[q];
        if (a.log_mel) a.log_mel[at] = logf(fmaxf(acc[q], a.floor));
      }
    }
  }
}

struct DistArgs {
  const float* la; const float* lb; const float* ma; const float* mb; const float* dct;
  const int64_t* frame_off; double* out;
  long long stride;
  int n_mels, n_mcep, nb;
};

constexpr double MT_DB = 4.3429448190325175;       // 10 / ln 10

__global__ __launch_bounds__(MT_THREADS) void metrics_distances_kernel(DistArgs a) {
  __shared__ double s_p[4][MT_THREADS];
  const int t = threadIdx.x;
  const long long i = blockIdx.x;
  const long long fo = (long long)a.frame_off[i];
  const long long F = (long long)a.frame_off[i + 1] - fo;
  double mae = 0.0, mcd = 0.0, num = 0.0, den = 0.0;
  for (long long e = t; e < F * a.n_mels; e += MT_THREADS) {
    const long long f = e / a.n_mels;
    const long long at = (e - f * a.n_mels) * a.stride + fo + f;
    mae += fabs((double)a.la[at] - (double)a.lb[at]);
  }
  for (long long f = t; f < F; f += MT_THREADS) {
    double s = 0.0;
    for (int q = 0; q < a.n_mcep; ++q) {
      double c = 0.0;
      for (int m = 0; m < a.n_mels; ++m) {
        const long long at = (long long)m * a.stride + fo + f;
        c += (double)a.dct[q * a.n_mels + m] * (0.5 * ((double)a.la[at] - (double)a.lb[at]));
      }
      s += c * c;
    }
    mcd += MT_DB * sqrt(2.0 * s);
  }
  for (long long e = t; e < F * a.nb; e += MT_THREADS) {
    const long long f = e / a.nb;
    const long long at = (e - f * a.nb) * a.stride + fo + f;
    const double va = (double)a.ma[at];
    const double d = va - (double)a.mb[at];
    num += d * d;
    den += va * va;
  }
  s_p[0][t] = mae; s_p[1][t] = mcd; s_p[2][t] = num; s_p[3][t] = den;
  __syncthreads();
  for (int h = MT_THREADS / 2; h >= 1; h >>= 1) {
    if (t < h) {
#pragma unroll
      for (int q = 0; q < 4; ++q) s_p[q][t] += s_p[q][t + h];
    }
    __syncthreads();
  }
  if (t == 0) {
    a.out[3 * i + 0] = s_p[0][0] / (double)(F * a.n_mels);
    a.out[3 * i + 1] = s_p[1][0] / (double)F;
    a.out[3 * i + 2] = sqrt(s_p[2][0]) / sqrt(s_p[3][0]);
  }
}

static bool metrics_desc_ok(const vqvae_metrics_desc* d) {
  return d && d->n >= 1 && d->ftot >= 1 && d->n_fft >= 32 && d->n_fft <= VQVAE_METRICS_MAX_NFFT && d->n_fft % 32 == 0 &&
         d->hop >= 1 && d->hop <= d->n_fft && d->n_mels >= 1 && d->n_mels <= VQVAE_METRICS_MAX_MELS && d->floor > 0.f && d->stride >= d->ftot;
}

// the one workspace plan of each entry point: nothing is taken today
struct MetricsPlan { size_t total; };
static MetricsPlan plan_stft_mel(const vqvae_metrics_desc*) { WsPlan p; return MetricsPlan{p.total}; }
static MetricsPlan plan_distances(const vqvae_metrics_desc*) { WsPlan p; return MetricsPlan{p.total}; }

}  // namespace vq

using namespace vq;

extern "C" int vqvae_metrics_abi_version(void) { return 1; }

extern "C" size_t vqvae_metrics_stft_mel_workspace_bytes(const vqvae_metrics_desc* d) {
  if (!metrics_desc_ok(d)) return (size_t)-1;
  return plan_stft_mel(d).total;
}

extern "C" size_t vqvae_metrics_distances_workspace_bytes(const vqvae_metrics_desc* d) {
  if (!metrics_desc_ok(d) || d->n_mcep < 1 || d->n_mcep >= d->n_mels) return (size_t)-1;
  return plan_distances(d).total;
}

#define MT_REQUIRE_DESC(who, d)                                                                                            \
  VQ_REQUIRE(d, who ": null descriptor");                                                                                  \
  VQ_REQUIRE(d->n >= 1, who ": n must be at least 1 (got %d)", (int)d->n);                                                 \
  VQ_REQUIRE(d->ftot >= 1, who ": ftot must be at least 1 (got %lld)", (long long)d->ftot);                                \
  VQ_REQUIRE(d->n_fft >= 32 && d->n_fft <= VQVAE_METRICS_MAX_NFFT && d->n_fft % 32 == 0,                                   \
             who ": n_fft must be a multiple of 32 in [32, %d] (got %d)", VQVAE_METRICS_MAX_NFFT, (int)d->n_fft);          \
  VQ_REQUIRE(d->hop >= 1 && d->hop <= d->n_fft, who ": hop must be in [1, n_fft] (got %d)", (int)d->hop);                  \
  VQ_REQUIRE(d->n_mels >= 1 && d->n_mels <= VQVAE_METRICS_MAX_MELS, who ": n_mels must be in [1, %d] (got %d)",            \
             VQVAE_METRICS_MAX_MELS, (int)d->n_mels);                                                                      \
  VQ_REQUIRE(d->floor > 0.f, who ": floor must be positive (got %g)", (double)d->floor);                                   \
  VQ_REQUIRE(d->stride >= d->ftot, who ": stride must be at least ftot (got %lld of %lld)", (long long)d->stride,          \
             (long long)d->ftot)

extern "C" int vqvae_metrics_stft_mel(const vqvae_metrics_desc* d, const float* x, const int64_t* off_in,
                                      const int64_t* frame_off, const float* dft, const float* mel, float* log_mel,
                                      float* mag, float* mel_pw, void* ws, size_t ws_bytes, vqvae_stream_t stream) {
  MT_REQUIRE_DESC("metrics_stft_mel", d);
  VQ_REQUIRE(x && off_in && frame_off && dft && mel, "metrics_stft_mel: null x, off_in, frame_off, dft or mel");
  VQ_REQUIRE(log_mel || mag || mel_pw, "metrics_stft_mel: log_mel, mag and mel_pw are all null");
  VQ_REQUIRE((reinterpret_cast<uintptr_t>(dft) & 15) == 0, "metrics_stft_mel: dft must be 16-byte aligned");
  const long long tiles = (d->ftot + MT_TILE - 1) / MT_TILE;
  VQ_REQUIRE(tiles <= 0x7fffffffLL, "metrics_stft_mel: %lld frames are more than 2^31 - 1 frame tiles", (long long)d->ftot);
  const MetricsPlan plan = plan_stft_mel(d);
  VQ_REQUIRE(ws_bytes >= plan.total && (ws || !plan.total), "metrics_stft_mel: workspace of %zu bytes, %zu needed", ws_bytes, plan.total);
  StftArgs a{};
  a.x = x; a.off_in = off_in; a.frame_off = frame_off; a.dft = dft; a.mel = mel; a.log_mel = log_mel; a.mag = mag; a.mel_pw = mel_pw;
  a.ftot = d->ftot; a.stride = d->stride; a.n = d->n; a.n_fft = d->n_fft; a.hop = d->hop; a.n_mels = d->n_mels; a.nb = d->n_fft / 2 + 1;
  a.floor = d->floor;
  size_t lds = mt_lds_staged(a.n_fft, a.hop, a.nb);
  a.stage_ok = lds <= MT_LDS_CAP ? 1 : 0;
  if (!a.stage_ok) lds = mt_lds_direct(a.nb);
  if (int e = lds_opt_in<metrics_stft_mel_kernel>(lds)) return e;
  hipLaunchKernelGGL(metrics_stft_mel_kernel, dim3((unsigned)tiles), dim3(MT_THREADS), lds, (hipStream_t)stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_metrics_distances(const vqvae_metrics_desc* d, const float* log_mel_a, const float* log_mel_b,
                                       const float* mag_a, const float* mag_b, const float* dct, const int64_t* frame_off,
                                       double* out, void* ws, size_t ws_bytes, vqvae_stream_t stream) {
  MT_REQUIRE_DESC("metrics_distances", d);
  VQ_REQUIRE(d->n_mcep >= 1 && d->n_mcep < d->n_mels, "metrics_distances: n_mcep must be in [1, n_mels) (got %d of %d)",
             (int)d->n_mcep, (int)d->n_mels);
  VQ_REQUIRE(log_mel_a && log_mel_b && mag_a && mag_b && dct && frame_off && out,
             "metrics_distances: null log_mel_a, log_mel_b, mag_a, mag_b, dct, frame_off or out");
  const MetricsPlan plan = plan_distances(d);
  VQ_REQUIRE(ws_bytes >= plan.total && (ws || !plan.total), "metrics_distances: workspace of %zu bytes, %zu needed", ws_bytes, plan.total);
  DistArgs a{};
  a.la = log_mel_a; a.lb = log_mel_b; a.ma = mag_a; a.mb = mag_b; a.dct = dct; a.frame_off = frame_off; a.out = out;
  a.stride = d->stride; a.n_mels = d->n_mels; a.n_mcep = d->n_mcep; a.nb = d->n_fft / 2 + 1;
  hipLaunchKernelGGL(metrics_distances_kernel, dim3((unsigned)d->n), dim3(MT_THREADS), 0, (hipStream_t)stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}
