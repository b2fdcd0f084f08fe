/*
 * fnet.h -- the launch plan of the float32 network kernels (fnet_kernels.hip, fnet_windows_kernels.hip), built by its host side (edison_fnet.hip) from an .ednf
 * blob (edison_amd/cube_import.py: version 1 without pads, version 2 with a conv's and a pool's (top, left, bottom, right) pads in
 * ints [16..23] of its 24-int records). Not part of the public ABI.
 */
#ifndef EDISON_FNET_H
#define EDISON_FNET_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#define ED_FNET_MAX_LAYERS 16
#define ED_FNET_THREADS 512
#define ED_FNET_MAX_BATCH 16                  /* utterances per workgroup, at most */
#define ED_FNET_LDS_BYTES (160 * 1024)
#define ED_FNET_ORIGIN_BIAS 4096              /* a padded record's rowin entry: (y0 + bias) << 16 | (x0 + bias) */
/* the layer road (fnet_layer_kernels.hip): a workgroup's tile of one record is MB rows x NB channels, its
 * operands pass through LDS in chunks of KC k */
#define ED_FNET_LAYER_MB 128
#define ED_FNET_LAYER_NB 64
#define ED_FNET_LAYER_KC 64
#define ED_FNET_LAYER_SA (ED_FNET_LAYER_KC + 2)   /* LDS row strides of A and B: the operand reads are conflict-free */
#define ED_FNET_LAYER_SB (ED_FNET_LAYER_NB + 16)
#define ED_FNET_LAYER_LDS_BYTES (4 * (ED_FNET_LAYER_MB * ED_FNET_LAYER_SA + ED_FNET_LAYER_KC * ED_FNET_LAYER_SB + 3 * ED_FNET_LAYER_MB))
#define ED_FNET_WORKSPACE_DEFAULT ((size_t)256 << 20) /* cap of the layer road's activation scratch (edison_fnet_set_workspace) */

/* One conv record (a dense layer is a conv whose kernel covers its whole input). Output row r of an utterance is element e = r % P of
 * the pool window of pooled position q = r / P (q = y * out_w + x, P = ph * pw): the P rows of a window are adjacent, so they land in
 * one lane's accumulator registers and the pool is a max over registers.
 * A record with a conv or a pool pad (pad = 1) has two more things in its tables. Its rowin entry is the row's
 * window origin (y0, x0) in input coordinates, packed with ED_FNET_ORIGIN_BIAS because a padded origin may be negative, or -1 for an
 * absent row: an element of a pool window that lies in the pool's padding, which is never read, written or counted and is -inf in the
 * window's max. And behind koff[k_pad] lies kyx[k_pad], (ky << 16 | kx) of every k: a tap is read only where (y0 + ky, x0 + kx) is
 * inside the in_h x in_w image, any other tap is the operand +0.0f. */
typedef struct {
	int32_t in_n, out_c, out_n;     /* in_h * in_w * in_c, out channels, out_h * out_w * out_c */
	int32_t P;                      /* pool window elements: 1, 2 or 4                          */
	int32_t rows;                   /* out_h * out_w * P output rows per utterance              */
	int32_t k_pad, n_pad;           /* K = kh * kw * in_c rounded up to 4, out_c up to 16       */
	int32_t relu;
	int32_t src, dst;               /* LDS activation buffer read / written (0 or 1)            */
	int32_t koff_at, rowin_at;      /* int32 offsets into tab: koff[k_pad], rowin[rows]          */
	int32_t acts_at;                /* float offset of this layer's output in a per-layer dump  */
	int32_t pad;                    /* 1: a padded record (origins in rowin, kyx behind koff)   */
	int32_t in_h, in_w, in_c;       /* the input image (read by padded records only)            */
	int32_t live;                   /* rows per utterance that are not absent (rows when pad = 0) */
	int64_t w_at;                   /* float offset into w: B[k_pad][n_pad], then bias[n_pad]   */
} ed_fnet_layer_t;

typedef struct {
	int32_t n_layers;               /* conv records; the last one's output goes through softmax */
	int32_t in_n, n_out;            /* network input / output floats per utterance              */
	int32_t batch;                  /* utterances per workgroup                                  */
	int32_t buf_n[2];               /* floats per utterance of LDS activation buffers 0 and 1   */
	int32_t w_lds, k_lds;           /* largest layer's B + koff (+ kyx) in LDS (floats / ints)  */
	int32_t acts_n;                 /* floats per utterance of a per-layer dump                 */
	const float *w;
	const int32_t *tab;
	ed_fnet_layer_t L[ED_FNET_MAX_LAYERS];
} ed_fnet_plan_t;

/* Dynamic LDS bytes of the plan's workgroup. */
static inline size_t ed_fnet_lds_bytes(const ed_fnet_plan_t *p)
{
	return sizeof(float) * ((size_t)p->batch * (size_t)(p->buf_n[0] + p->buf_n[1]) + (size_t)p->w_lds) + sizeof(int32_t) * (size_t)p->k_lds;
}

/* Whether a launcher may start the plan's workgroup with lds bytes of dynamic LDS (its own sum: ed_fnet_lds_bytes, or more behind it). */
static inline int ed_fnet_plan_launchable(const ed_fnet_plan_t *p, size_t lds)
{
	return lds <= ED_FNET_LDS_BYTES && p->batch >= 1 && p->n_layers >= 1 && p->n_layers <= ED_FNET_MAX_LAYERS;
}

/* n utterances -> logits / probs [n][n_out] (NULL: not written), argmax [n] (NULL: not written); acts != NULL also dumps every layer's
 * output [n][acts_n]. Utterance u is the in_n floats at in + u * in_stride: in_stride = in_n for inputs back to back, num_mfcc for the
 * overlapping windows of a stream's feature rows (edison_stream_float). Returns a hipError_t. */
extern "C" int ed_launch_fnet(const ed_fnet_plan_t *p, const float *in, int64_t in_stride, int64_t n, float *logits, float *probs, int32_t *argmax,
                              float *acts, hipStream_t stream);
/* The windows of a bank of microphones (fnet_windows_kernels.hip): utterance U < n * n_mics (< 2^31) is frame i = U / n_mics of
 * microphone m = U % n_mics, the in_n floats at in + m * mic_stride + i * frame_stride; outputs [n][n_mics][..], row U (NULL: not written).
 * One launch. per_frame != 0 (tools/bench_float_bank.py only; the library passes 0): n launches of ed_launch_fnet instead, one per frame
 * over its n_mics windows, which computes the same outputs. Returns a hipError_t. */
extern "C" int ed_launch_fnet_windows(const ed_fnet_plan_t *p, const float *in, int64_t mic_stride, int32_t n_mics, int64_t frame_stride, int32_t n,
                                      float *logits, float *probs, int32_t *argmax, int per_frame, hipStream_t stream);
/* The layer road: a plan with batch = 0 (a layered network, edison_fnet_load_ex) runs one launch of ed_fnet_layer_kernel per record
 * and one softmax launch per chunk of at most `chunk` utterances: (n_layers + 1) * ceil(n / chunk) launches. Record l reads
 * [nu][buf_n[src]] from ws[src] and writes [nu][buf_n[dst]] to ws[dst]; the first record reads `in` in place. ws[i] holds
 * chunk * buf_n[i] floats. ms != NULL (tools/bench_fnet_large.py): [n_layers + 1] receives each launch's milliseconds, summed over the
 * chunks, and the stream is synchronised after every chunk. Returns a hipError_t. */
extern "C" int ed_launch_fnet_layered(const ed_fnet_plan_t *p, const float *in, int64_t n, int64_t chunk, float *const ws[2], float *logits, float *probs,
                                      int32_t *argmax, float *acts, float *ms, hipStream_t stream);
/* The context's loaded float network's plan, NULL when none is loaded (edison_fnet.hip). */
struct edison_ctx;
const ed_fnet_plan_t *ed_ctx_fnet_plan(const struct edison_ctx *ctx);
/* Whether the loaded network is a layered one (plan batch 0): every consumer of the plan that runs the in-LDS kernels refuses it by
 * name with ed_fnet_refuse_layered (EDISON_E_NO_IMPL, "<who>: ... layer road ..."). */
int ed_ctx_fnet_layered(const struct edison_ctx *ctx);
int ed_fnet_refuse_layered(struct edison_ctx *ctx, const char *who);
/* What the plan's tables leave out of a conv record's geometry, for host code that builds tables of its own (the BatchNorm trainer's
 * rows over the whole conv map, edison_ftrain.hip): strides, the pool window, the conv's map ch x cw before the pool and the pooled
 * map oh x ow. [n_layers] of the loaded network, NULL when none is loaded. */
typedef struct {
	int32_t sh, sw, ph, pw, ch, cw, oh, ow;
} ed_fnet_geom_t;
const ed_fnet_geom_t *ed_ctx_fnet_geom(const struct edison_ctx *ctx);
/* The host flow's net input: out[i] = min(max((float)y[i] * scale, lo), hi) for i < count. Returns a hipError_t. */
extern "C" int ed_launch_fnet_input(const double *y, int64_t count, float scale, float lo, float hi, float *out, int n_cu, hipStream_t stream);

#endif
