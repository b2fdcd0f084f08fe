/*
 * edison_stream_core.hip -- the sliding-window core of the any-geometry streams (edison_stream_core.h): the two
 * state kernels, one workgroup per microphone, and the host logic around them that the two front ends, one per network type
 * (edison_stream_bank.hip, edison_float_bank.hip; sections 12b, 15a), share. The microphone count and a push's mask are
 * data of the launch: a single stream is a bank of one microphone and runs the same kernels at grid 1.
 */
#include <math.h>
#include <string.h>

#include "edison_stream_core.h"

/* Workgroup m moves microphone m's history -- the newest `tail` samples from a_src and feat_bytes bytes from f_src -- to the front of its
 * buffers, a_stride samples and f_stride bytes behind microphone m - 1's. The destination lies BELOW the source and may overlap it: in
 * rounds of 256 elements every lane reads, the workgroup waits, every lane writes. A write to element j clobbers source element
 * j - src < j, which this round or an earlier one has already read. */
__global__ __launch_bounds__(256) void ed_stream_core_shift_kernel(int16_t *audio, int64_t a_stride, int64_t a_src, int tail, int8_t *feat,
                                                                   int64_t f_stride, int64_t f_src, int feat_bytes)
{
	const int t = threadIdx.x;
	audio += (int64_t)blockIdx.x * a_stride;
	feat += (int64_t)blockIdx.x * f_stride;
	for (int base = 0; base < tail; base += 256)
	{
		const int j = base + t;
		const int16_t v = j < tail ? audio[a_src + j] : (int16_t)0;
		__syncthreads();
		if (j < tail) audio[j] = v;
		__syncthreads();
	}
	for (int base = 0; base < feat_bytes; base += 256)
	{
		const int j = base + t;
		const int8_t v = j < feat_bytes ? feat[f_src + j] : (int8_t)0;
		__syncthreads();
		if (j < feat_bytes) feat[j] = v;
		__syncthreads();
	}
}

/*
 * The firmware's post-processing (app.c:332-356) over n_out classes, for the n inferences of a push; workgroup m serves microphone m:
 *   state[c] = ed_filter_step(alpha, state[c], ed_filter_term(1 - alpha, x[c]))   the arithmetic and its rounding: edison_postproc_core.h
 *   likely = first maximum of the state row, spotted = likely if that maximum > threshold, else -1;   then edisonFSM on lane 0
 * The recurrence is sequential in time; classes run on lanes, the per-frame maximum afterwards on frames. Entry i of microphone m is row
 * i * n_mics + m of the time-major arrays x / filt [n][n_mics][n_out] and likely / spotted / fs.states [n][n_mics]; between pushes the
 * microphone keeps state [n_mics][n_out] and fs.fsm [n_mics]. A single stream is the bank of one: m = 0, n_mics = gridDim.x = 1.
 * T = int8_t: the int8 graph's softmax / logits; T = float: the float network's probabilities. (double)x is exact for both.
 * present [n_mics] (NULL: everyone): a microphone the push left out gets the fill -- zero bytes in its rows of filt, -1 in likely and
 * spotted, its machine's unchanged state in fs.states, the unchanged machine in fs.copy -- and keeps state[m] and fs.fsm[m].
 */
template <class T>
__global__ __launch_bounds__(256) void ed_stream_core_filter_kernel(const unsigned char *present, const T *x, int n, int n_out, double alpha,
                                                                    double one_minus_alpha, double threshold, float *state, float *filt,
                                                                    int32_t *likely, int32_t *spotted, ed_fsm_stage_t fs)
{
	const int t = threadIdx.x;
	const size_t m = blockIdx.x, n_mics = gridDim.x;
	if (present && !present[m])
	{
		/* the rows of filt: 256 / n_out rows a round, a lane per element, so that a row's stores are adjacent (n_out <= 256, one
		 * 32-bit division per lane); the machine is read in place, not into a local copy */
		const int per = 256 / n_out, r = t / n_out, c = t % n_out;
		for (int i = r; i < n && r < per; i += per) filt[(i * n_mics + m) * n_out + c] = 0.0f;
		const int held = fs.fsm ? fs.fsm[m].state : 0;
		for (int i = t; i < n; i += 256)
		{
			const size_t im = i * n_mics + m;
			likely[im] = -1;
			spotted[im] = -1;
			if (fs.fsm) fs.states[im] = held;
		}
		if (fs.fsm && fs.copy && t == 0) fs.copy[m] = fs.fsm[m];
		return;
	}
	if (t < n_out)
	{
		float y = state[m * n_out + t];
		for (int i = 0; i < n; i++)
		{
			const size_t at = (i * n_mics + m) * n_out + t;
			y = ed_filter_step(alpha, y, ed_filter_term(one_minus_alpha, (double)x[at]));
			filt[at] = y;
		}
		state[m * n_out + t] = y;
	}
	__syncthreads();
	for (int i = t; i < n; i += 256)
	{
		const size_t im = i * n_mics + m;
		const float *row = filt + im * n_out;
		float best = row[0];
		int idx = 0;
		for (int c = 1; c < n_out; c++)
			if (best < row[c]) { best = row[c]; idx = c; }
		likely[im] = idx;
		spotted[im] = ((double)best > threshold) ? idx : -1;
	}
	if (!fs.fsm) return;
	__syncthreads();
	if (t == 0)
	{
		edison_fsm mach = fs.fsm[m];
		for (int i = 0; i < n; i++)
		{
			const size_t im = i * n_mics + m;
			fs.states[im] = ed_fsm_step_core(&mach, spotted[im] >= 0, (uint32_t)likely[im], fs.dt_us, &fs.roles);
		}
		fs.fsm[m] = mach;
		if (fs.copy) fs.copy[m] = mach;
	}
}

/* `code` with "<who>: <what>" in ctx->err */
static int core_err(edison_ctx *ctx, const char *who, int code, const char *what)
{
	snprintf(ctx->err, sizeof(ctx->err), "%s: %s", who, what);
	return code;
}

/* Work the stream left unsynchronised on another HIP stream must be behind us before q touches the stream's state. */
static int order_after(ed_stream_core *c, hipStream_t q)
{
	if (!c->q_pending || c->q_last == q) return EDISON_OK;
	if (hipEventRecord(c->ev, c->q_last) == hipSuccess) ED_HIP(c->ctx, hipStreamWaitEvent(q, c->ev, 0));
	else (void)hipGetLastError(); /* the caller destroyed that stream (which drains it) */
	c->q_pending = 0;
	return EDISON_OK;
}

/* Before a push of n frames: the history to the front when the push would run past the end of the buffers. */
static int make_room(ed_stream_core *c, hipStream_t q, int n)
{
	if (c->pos + n <= c->slots * c->chunk || c->pos == 0) return EDISON_OK;
	const int64_t a_src = (int64_t)c->pos * c->hop, f_src = (int64_t)c->pos * c->nm * c->feat_elem;
	const int feat_bytes = c->feat_elem * (c->F - 1) * c->nm;
	hipLaunchKernelGGL(ed_stream_core_shift_kernel, dim3(c->n_mics), dim3(256), 0, q, c->d_audio, (int64_t)c->mic_audio, a_src, c->tail,
	                   (int8_t *)c->d_feat, (int64_t)c->mic_feat, f_src, feat_bytes);
	c->pos = 0;
	return hipGetLastError() == hipSuccess ? EDISON_OK : core_err(c->ctx, c->who, EDISON_E_RUNTIME, "shift launch failed");
}

int ed_stream_core_check_opts(edison_ctx *ctx, const char *who, const edison_kws_geom *g, const ed_stream_core_opts *o)
{
	if (o->chunk_frames < 1) return core_err(ctx, who, EDISON_E_ARGUMENT, "chunk_frames >= 1");
	/* positions and sample counts are ints in places (pos * hop, kernel arguments): as edison_stream_create_ex */
	if ((int64_t)o->chunk_frames * g->frame_step >= ((int64_t)1 << 30))
		return core_err(ctx, who, EDISON_E_SIZE, "chunk_frames x frame_step must stay below 2^30 samples per push");
	if (o->fsm && !o->filter) return core_err(ctx, who, EDISON_E_ARGUMENT, "the state machine (fsm) works on the filtered outputs: filter = 1 too");
	if (o->filter && !(o->filter_alpha >= 0.0 && o->filter_alpha <= 1.0))
		return core_err(ctx, who, EDISON_E_ARGUMENT, "filter_alpha must be within [0, 1]");
	return EDISON_OK;
}

int ed_stream_core_create(ed_stream_core *c, edison_ctx *ctx, const char *who, int feat_elem, int out_elem, const edison_kws_geom *g, int F,
                          int n_out, int n_mics, const ed_stream_core_opts *o, size_t front_bytes)
{
	c->ctx = ctx; c->who = who; c->feat_elem = feat_elem; c->out_elem = out_elem; c->n_mics = n_mics;
	c->F = F; c->nm = g->num_mfcc; c->hop = g->frame_step; c->chunk = o->chunk_frames;
	c->tail = g->frame_len > g->frame_step ? g->frame_len - g->frame_step : 0;
	c->n_out = n_out;
	c->filter = o->filter ? 1 : 0; c->fsm = o->fsm ? 1 : 0;
	c->alpha = o->filter_alpha;
	c->one_minus_alpha = 1.0 - o->filter_alpha; /* folded in double, as the firmware's (1.0-NET_OUT_MOVING_AVG_ALPHA) */
	c->threshold = o->true_threshold;
	c->dt_us = (uint32_t)floor((double)g->frame_step * 1e6 / g->sample_rate);
	edison_fsm_roles(&c->roles.wake_idx, &c->roles.loc_mask, &c->roles.val_mask);

	ED_HIP(ctx, hipSetDevice(ctx->device));
	hipError_t e = hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking);
	if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev, hipEventDisableTiming);
	/* eight pushes of room while that stays within 64 MB of samples, else one (then every push after the first shifts) */
	const size_t n = (size_t)c->chunk, push_samples = n * (size_t)c->hop;
	c->slots = push_samples * sizeof(int16_t) * ED_STREAM_CORE_SLOTS <= ED_STREAM_CORE_SLOTS_BYTES ? ED_STREAM_CORE_SLOTS : 1;
	const size_t mics = (size_t)n_mics, nt = n * mics; /* entries per push of the time-major outputs */
	c->mic_audio = ed_stream_core_mic_audio(c->tail, c->slots, c->chunk, c->hop);
	c->mic_feat = ed_stream_core_mic_feat(c->feat_elem, c->F, c->slots, c->chunk, c->nm);
	if (e == hipSuccess) e = hipMalloc((void **)&c->d_audio, sizeof(int16_t) * mics * c->mic_audio + ED_STREAM_CORE_SLACK);
	if (e == hipSuccess) e = hipMalloc((void **)&c->d_feat, mics * c->mic_feat + ED_STREAM_CORE_SLACK);
	size_t off = ed_stream_core_align(front_bytes);
	c->off_filt = off; off += c->filter ? nt * (size_t)c->n_out * sizeof(float) : 0;
	c->off_likely = off; off += c->filter ? nt * sizeof(int32_t) : 0;
	c->off_spotted = off; off += c->filter ? nt * sizeof(int32_t) : 0;
	c->off_states = off; off += c->fsm ? nt * sizeof(int32_t) : 0;
	off = ed_stream_core_align(off); c->off_fsm = off; off += c->fsm ? mics * sizeof(edison_fsm) : 0;
	c->out_bytes = off;
	if (e == hipSuccess) e = hipMalloc((void **)&c->d_out, c->out_bytes);
	if (e == hipSuccess) e = hipHostMalloc((void **)&c->h_out, c->out_bytes, hipHostMallocDefault);
	if (e == hipSuccess) e = hipHostMalloc((void **)&c->h_in, sizeof(int16_t) * mics * push_samples + mics, hipHostMallocDefault);
	if (e == hipSuccess) c->h_present = (unsigned char *)(c->h_in + mics * push_samples);
	if (e == hipSuccess) e = hipMalloc((void **)&c->d_missed, mics * sizeof(int64_t) + mics);
	if (e == hipSuccess) c->d_present = (unsigned char *)(c->d_missed + mics);
	if (e == hipSuccess && c->filter) e = hipMalloc((void **)&c->d_state, sizeof(float) * mics * (size_t)c->n_out);
	if (e == hipSuccess && c->fsm) e = hipMalloc((void **)&c->d_fsm, mics * sizeof(edison_fsm));
	if (e != hipSuccess)
	{
		(void)hipGetLastError();
		return core_err(ctx, who, e == hipErrorOutOfMemory ? EDISON_E_NO_MEMORY : EDISON_E_RUNTIME, "allocation failed");
	}
	return ed_stream_core_reset(c);
}

void ed_stream_core_free(ed_stream_core *c)
{
	if (c->own && c->ev) (void)order_after(c, c->own);
	if (c->own) (void)hipStreamSynchronize(c->own);
	if (c->d_audio) (void)hipFree(c->d_audio);
	if (c->d_feat) (void)hipFree(c->d_feat);
	if (c->d_out) (void)hipFree(c->d_out);
	if (c->d_state) (void)hipFree(c->d_state);
	if (c->d_fsm) (void)hipFree(c->d_fsm);
	if (c->d_missed) (void)hipFree(c->d_missed);
	if (c->h_in) (void)hipHostFree(c->h_in);
	if (c->h_out) (void)hipHostFree(c->h_out);
	if (c->ev) (void)hipEventDestroy(c->ev);
	if (c->own) (void)hipStreamDestroy(c->own);
}

/* On the stream's own HIP stream: the history of microphones m .. m + count - 1 at the current pos (`tail` samples, F - 1 rows; float
 * rows: +0.0f), their filter states and their state machines to the start values. */
static int start_state(ed_stream_core *c, int m, int count)
{
	edison_ctx *ctx = c->ctx;
	int16_t *audio = c->d_audio + (size_t)m * c->mic_audio + (size_t)c->pos * c->hop;
	unsigned char *feat = c->d_feat + (size_t)m * c->mic_feat + (size_t)c->pos * c->nm * c->feat_elem;
	const size_t tail_bytes = sizeof(int16_t) * (size_t)c->tail, hist_bytes = (size_t)c->feat_elem * (size_t)(c->F - 1) * c->nm;
	if (count == 1)
	{
		if (tail_bytes) ED_HIP(ctx, hipMemsetAsync(audio, 0, tail_bytes, c->own));
		if (hist_bytes) ED_HIP(ctx, hipMemsetAsync(feat, 0, hist_bytes, c->own));
	}
	else
	{
		if (tail_bytes) ED_HIP(ctx, hipMemset2DAsync(audio, sizeof(int16_t) * c->mic_audio, 0, tail_bytes, (size_t)count, c->own));
		if (hist_bytes) ED_HIP(ctx, hipMemset2DAsync(feat, c->mic_feat, 0, hist_bytes, (size_t)count, c->own));
	}
	if (c->filter) ED_HIP(ctx, hipMemsetAsync(c->d_state + (size_t)m * c->n_out, 0, sizeof(float) * (size_t)count * c->n_out, c->own));
	if (c->fsm)
	{
		edison_fsm start;
		edison_fsm_init(&start); /* EDI_RESET, as the firmware enters its continuous loop (app.c:288-300) */
		for (int i = 0; i < count; i++)
			ED_HIP(ctx, hipMemcpyAsync(c->d_fsm + m + i, &start, sizeof(start), hipMemcpyHostToDevice, c->own));
	}
	return EDISON_OK;
}

int ed_stream_core_reset_mic(ed_stream_core *c, int mic)
{
	if (!c) return EDISON_E_ARGUMENT;
	if (mic < 0 || mic >= c->n_mics) return core_err(c->ctx, c->who, EDISON_E_ARGUMENT, "microphone index out of range");
	{ const int r = order_after(c, c->own); if (r != EDISON_OK) return r; }
	{ const int r = start_state(c, mic, 1); if (r != EDISON_OK) return r; }
	ED_HIP(c->ctx, hipStreamSynchronize(c->own));
	c->q_pending = 0;
	return EDISON_OK;
}

int ed_stream_core_reset(ed_stream_core *c)
{
	if (!c) return EDISON_E_ARGUMENT;
	edison_ctx *ctx = c->ctx;
	{ const int r = order_after(c, c->own); if (r != EDISON_OK) return r; }
	c->pos = 0;
	{ const int r = start_state(c, 0, c->n_mics); if (r != EDISON_OK) return r; }
	ED_HIP(ctx, hipMemsetAsync(c->d_out, 0, c->out_bytes, c->own));
	ED_HIP(ctx, hipMemsetAsync(c->d_missed, 0, (size_t)c->n_mics * sizeof(int64_t), c->own));
	ED_HIP(ctx, hipStreamSynchronize(c->own));
	memset(c->h_out, 0, c->out_bytes);
	c->q_pending = 0;
	c->last_n = c->chunk;
	c->last_staged = 0;
	c->frames_seen = 0;
	return EDISON_OK;
}

int ed_stream_core_begin_push(ed_stream_core *c, hipStream_t q, const int16_t *samples, int n, int host)
{
	if (n < 1 || n > c->chunk) return core_err(c->ctx, c->who, EDISON_E_ARGUMENT, "n_frames must be 1 .. chunk_frames");
	{ const int r = order_after(c, q); if (r != EDISON_OK) return r; }
	{ const int r = make_room(c, q, n); if (r != EDISON_OK) return r; }
	const size_t bytes = sizeof(int16_t) * (size_t)n * c->hop;
	if (host) memcpy(c->h_in, samples, bytes * (size_t)c->n_mics);
	int16_t *dst = c->d_audio + (size_t)c->pos * c->hop + c->tail;
	const int16_t *src = host ? c->h_in : samples;
	const hipMemcpyKind kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
	if (c->n_mics == 1) ED_HIP(c->ctx, hipMemcpyAsync(dst, src, bytes, kind, q));
	else ED_HIP(c->ctx, hipMemcpy2DAsync(dst, sizeof(int16_t) * c->mic_audio, src, bytes, bytes, (size_t)c->n_mics, kind, q)); /* a row per microphone */
	return EDISON_OK;
}

/* Where the stream has a filter: the filter (+ edisonFSM, writing into the output block) over fin [n][n_mics][n_out], a workgroup per
 * microphone; present: the push's mask in device memory, NULL: every microphone. */
static int launch_filter(ed_stream_core *c, hipStream_t q, const unsigned char *present, const void *fin, int n)
{
	if (!c->filter) return EDISON_OK;
	unsigned char *o = c->d_out;
	ed_fsm_stage_t fs;
	memset(&fs, 0, sizeof(fs));
	if (c->fsm)
	{
		fs.fsm = c->d_fsm; fs.states = (int32_t *)(o + c->off_states); fs.copy = (edison_fsm *)(o + c->off_fsm);
		fs.dt_us = c->dt_us; fs.roles = c->roles;
	}
	float *filt = (float *)(o + c->off_filt);
	int32_t *likely = (int32_t *)(o + c->off_likely), *spotted = (int32_t *)(o + c->off_spotted);
	if (c->out_elem == 1)
		hipLaunchKernelGGL(ed_stream_core_filter_kernel<int8_t>, dim3(c->n_mics), dim3(256), 0, q, present, (const int8_t *)fin, n, c->n_out, c->alpha,
		                   c->one_minus_alpha, c->threshold, c->d_state, filt, likely, spotted, fs);
	else
		hipLaunchKernelGGL(ed_stream_core_filter_kernel<float>, dim3(c->n_mics), dim3(256), 0, q, present, (const float *)fin, n, c->n_out, c->alpha,
		                   c->one_minus_alpha, c->threshold, c->d_state, filt, likely, spotted, fs);
	return hipGetLastError() == hipSuccess ? EDISON_OK : core_err(c->ctx, c->who, EDISON_E_RUNTIME, "filter launch failed");
}

/* behind the filter of a push of n frames: pos, the host push's download and wait, what the getters need to know */
static int end_push(ed_stream_core *c, hipStream_t q, int n, int host)
{
	c->pos += n;
	if (host)
	{
		ED_HIP(c->ctx, hipMemcpyAsync(c->h_out, c->d_out, c->out_bytes, hipMemcpyDeviceToHost, q));
		ED_HIP(c->ctx, hipStreamSynchronize(q));
	}
	else c->q_last = q;
	c->q_pending = !host;
	c->last_n = n;
	c->last_staged = host;
	c->frames_seen += n;
	return EDISON_OK;
}

int ed_stream_core_finish_push(ed_stream_core *c, hipStream_t q, const void *fin, int n, int host)
{
	{ const int r = launch_filter(c, q, NULL, fin, n); if (r != EDISON_OK) return r; }
	return end_push(c, q, n, host);
}

int ed_stream_core_finish_push_present(ed_stream_core *c, hipStream_t q, const void *fin, int n, int host, const unsigned char *present, void *out0,
                                       void *out1, int32_t *argmax)
{
	if (host)
	{
		/* the pushes before this one on q have been waited for (a host push ends with a wait), so h_present is free */
		memcpy(c->h_present, present, (size_t)c->n_mics);
		ED_HIP(c->ctx, hipMemcpyAsync(c->d_present, c->h_present, (size_t)c->n_mics, hipMemcpyHostToDevice, q));
		present = c->d_present;
	}
	ed_bank_hold_t h;
	memset(&h, 0, sizeof(h));
	h.present = present;
	h.audio = c->d_audio; h.a_stride = (int64_t)c->mic_audio; h.a_src = (int64_t)c->pos * c->hop; h.a_by = (int64_t)n * c->hop; h.tail = c->tail;
	h.feat = (int8_t *)c->d_feat; h.f_stride = (int64_t)c->mic_feat;
	h.f_src = (int64_t)c->pos * c->nm * c->feat_elem; h.f_by = (int64_t)n * c->nm * c->feat_elem; h.feat_bytes = c->feat_elem * (c->F - 1) * c->nm;
	h.n = n; h.row_bytes = c->n_out * c->out_elem;
	h.out0 = (unsigned char *)out0; h.out1 = (unsigned char *)out1; h.argmax = argmax;
	h.missed = c->d_missed;
	ed_bank_launch_hold(q, c->n_mics, &h);
	if (hipGetLastError() != hipSuccess) return core_err(c->ctx, c->who, EDISON_E_RUNTIME, "hold launch failed");
	{ const int r = launch_filter(c, q, present, fin, n); if (r != EDISON_OK) return r; }
	return end_push(c, q, n, host);
}

int ed_stream_core_frames_seen_mics(ed_stream_core *c, int64_t *counts)
{
	if (!c || !counts) return EDISON_E_ARGUMENT;
	{ const int r = order_after(c, c->own); if (r != EDISON_OK) return r; }
	ED_HIP(c->ctx, hipMemcpyAsync(counts, c->d_missed, (size_t)c->n_mics * sizeof(int64_t), hipMemcpyDeviceToHost, c->own));
	ED_HIP(c->ctx, hipStreamSynchronize(c->own));
	c->q_pending = 0;
	for (int m = 0; m < c->n_mics; m++) counts[m] = c->frames_seen - counts[m];
	return EDISON_OK;
}

/* Copy `count` pieces of the last push's output block to the caller: from h_out after a host push, else from d_out on the stream the
 * work went to (host = 1: synchronously; host = 0: ordered on the context's stream). */
struct edsg_piece { void *dst; size_t off, bytes; };
static int copy_out(ed_stream_core *c, const edsg_piece *p, int count, int host)
{
	edison_ctx *ctx = c->ctx;
	if (host && c->last_staged)
	{
		for (int i = 0; i < count; i++)
			if (p[i].dst) memcpy(p[i].dst, c->h_out + p[i].off, p[i].bytes);
		return EDISON_OK;
	}
	hipStream_t q = host ? c->own : ctx->stream;
	{ const int r = order_after(c, q); if (r != EDISON_OK) return r; }
	for (int i = 0; i < count; i++)
		if (p[i].dst)
			ED_HIP(ctx, hipMemcpyAsync(p[i].dst, c->d_out + p[i].off, p[i].bytes, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, q));
	if (host) ED_HIP(ctx, hipStreamSynchronize(q));
	else c->q_last = q;
	c->q_pending = !host;
	return EDISON_OK;
}

int ed_stream_core_filtered(ed_stream_core *c, float *filt, int32_t *likely, int32_t *spotted, int host)
{
	if (!c) return EDISON_E_ARGUMENT;
	if (!c->filter) return core_err(c->ctx, c->who, EDISON_E_ARGUMENT, "created without the output filter");
	const size_t n = (size_t)c->last_n * (size_t)c->n_mics;
	const edsg_piece p[3] = {{filt, c->off_filt, n * (size_t)c->n_out * sizeof(float)}, {likely, c->off_likely, n * sizeof(int32_t)},
	                         {spotted, c->off_spotted, n * sizeof(int32_t)}};
	return copy_out(c, p, 3, host);
}

int ed_stream_core_fsm(ed_stream_core *c, edison_fsm *fsm, int32_t *states, int host)
{
	if (!c) return EDISON_E_ARGUMENT;
	if (!c->fsm) return core_err(c->ctx, c->who, EDISON_E_ARGUMENT, "created without the state machine (opts.fsm)");
	const size_t mics = (size_t)c->n_mics;
	const edsg_piece p[2] = {{states, c->off_states, (size_t)c->last_n * mics * sizeof(int32_t)}, {fsm, c->off_fsm, mics * sizeof(edison_fsm)}};
	return copy_out(c, p, 2, host);
}
