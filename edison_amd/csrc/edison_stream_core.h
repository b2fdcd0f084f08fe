/*
 * edison_stream_core.h -- the sliding-window core that edison_stream_bank.hip and edison_float_bank.hip run on (edison_stream_core.hip,
 * DESIGN.md section 12a): the state a continuous stream keeps between pushes and everything that does not depend on which MFCC and
 * which network fill the window. An owner holds one core by value, launches its features and its network between begin_push and
 * finish_push, and lays out the front of the output block. Not part of the public ABI.
 *
 * Two sliding buffers `slots` pushes long,
 *     d_audio  [T + slots * chunk * hop] int16                   T = `tail` samples of history, then the new samples
 *     d_feat   [F - 1 + slots * chunk][nm] of feat_elem bytes    F - 1 rows of history, then the new rows
 * whose history starts at frame `pos` (samples pos * hop, rows pos): a push appends behind it and advances pos by its frames; window i
 * of the push is rows pos + i .. pos + i + F - 1, read in place by the owner's network kernel. When the next push would run past the
 * end, the shift kernel first moves the history back to the front.
 *
 * A core serves n_mics microphones that advance in lockstep (1: an edison_stream_geom / edison_stream_float, or a bank of one; more: an
 * edison_stream_bank / edison_float_bank, DESIGN.md sections 12b and 15a). Each microphone has the two buffers above, mic_audio samples and mic_feat bytes behind its neighbour's, and all
 * share one pos. A push carries [n_mics][n * hop] samples; everything it puts out is time-major: filt [n][n_mics][n_out], likely /
 * spotted / states [n][n_mics], the machines [n_mics]. With n_mics = 1 the core issues the copies and launches it issued before it had
 * the dimension, with more one strided copy; the two state kernels (edison_stream_core.hip) run one workgroup per microphone either way.
 *
 * A push may leave microphones out (finish_push_present): pos advances for all of them, the hold kernel of
 * edison_bank_hold.hip carries an absent microphone's history forward to the new pos, and the filter kernel, given the mask, leaves
 * everything else the microphone owns as it was.
 */
#ifndef EDISON_STREAM_CORE_H
#define EDISON_STREAM_CORE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edison_ctx.h"
#include "edison_postproc_core.h"

#define EDSG_FILTER_MAX_OUT 256                       /* classes the filter kernel serves: one lane each in one workgroup */
#define ED_STREAM_CORE_SLOTS 8                        /* pushes of room in the sliding buffers ...                         */
#define ED_STREAM_CORE_SLOTS_BYTES ((size_t)64 << 20) /* ... while that many pushes of samples stay within 64 MB, else one */
#define ED_STREAM_CORE_SLACK 64                       /* bytes allocated behind d_audio and behind d_feat                  */
#define ED_STREAM_CORE_ALIGN 16                       /* alignment of the parts of the output block                        */

static inline size_t ed_stream_core_align(size_t off) { return (off + (ED_STREAM_CORE_ALIGN - 1)) & ~(size_t)(ED_STREAM_CORE_ALIGN - 1); }
/* one microphone's sliding buffers: samples of d_audio, bytes of d_feat */
static inline size_t ed_stream_core_mic_audio(int tail, int slots, int chunk, int hop) { return (size_t)tail + (size_t)slots * chunk * hop; }
static inline size_t ed_stream_core_mic_feat(int feat_elem, int F, int slots, int chunk, int nm)
{
	return (size_t)feat_elem * ((size_t)(F - 1) + (size_t)slots * chunk) * nm;
}

struct ed_stream_core
{
	edison_ctx *ctx;
	const char *who;               /* the owner's message prefix: "stream_geom", "stream_float", "stream_bank", "float_bank" */
	int feat_elem, out_elem;       /* bytes per feature element and per network output: 1 (the int8 graph) or 4 (the float network) */
	int F, nm, hop, tail, chunk;   /* frames per window, coefficients per row, frame_step, T history samples, frames per push */
	int n_out, filter, fsm;
	int n_mics;                    /* microphones in lockstep */
	size_t mic_audio, mic_feat;    /* from one microphone's buffer to the next: samples of d_audio, bytes of d_feat */
	double alpha, one_minus_alpha, threshold;
	ed_fsm_roles_t roles;
	uint32_t dt_us;
	int slots, pos;                /* buffers of `slots` pushes; the history starts at frame pos */
	int16_t *d_audio;
	unsigned char *d_feat;
	/* every output of a push in one block (device d_out, pinned h_out), so that a host push downloads once: the owner's in front */
	unsigned char *d_out, *h_out;
	size_t off_filt, off_likely, off_spotted, off_states, off_fsm, out_bytes;
	int16_t *h_in;                 /* pinned [n_mics][chunk * hop]: the host push's upload; behind it h_present */
	float *d_state;                /* [n_mics][n_out] the filter state */
	edison_fsm *d_fsm;             /* [n_mics] */
	hipStream_t own;               /* host pushes run here */
	hipEvent_t ev;
	hipStream_t q_last;            /* where the last unsynchronised work on the stream's state went (device pushes: the caller's stream) */
	int q_pending;
	int last_n, last_staged;       /* frames of the last push; 1: its outputs are in h_out already (host push) */
	int64_t frames_seen;
	/* pushes that leave microphones out (finish_push_present) */
	int64_t *d_missed;             /* [n_mics] frames of the pushes a microphone was absent from; behind it d_present */
	unsigned char *d_present;      /* [n_mics] where a host push's mask is uploaded */
	unsigned char *h_present;      /* pinned [n_mics], the tail of h_in's allocation */
};

/* A push of n frames that left microphones out, after its feature and network launches (edison_bank_hold.hip; one workgroup per
 * microphone, a microphone with present[m] != 0 is not touched). The absent microphone's garbage went to samples a_src + tail and later
 * and to feature bytes f_src + feat_bytes and later, so its history at a_src / f_src is intact: the hold moves it UP by a_by samples and
 * f_by bytes, to where the next push looks for it, zeroes its rows of the network outputs out0 / out1 [n][n_mics][row_bytes] (NULL: not
 * written), puts -1 into its argmax [n][n_mics] (NULL: none) and adds n to missed[m]. */
struct ed_bank_hold_t
{
	const unsigned char *present;  /* [n_mics] device memory */
	int16_t *audio;                /* microphone 0's buffer; a_stride samples to the next */
	int64_t a_stride, a_src, a_by;
	int tail;
	int8_t *feat;                  /* microphone 0's rows; f_stride bytes to the next */
	int64_t f_stride, f_src, f_by;
	int feat_bytes;
	int n, row_bytes;
	unsigned char *out0, *out1;
	int32_t *argmax;
	int64_t *missed;               /* [n_mics] */
};
void ed_bank_launch_hold(hipStream_t q, int n_mics, const ed_bank_hold_t *h);

/* the options both public option structs carry */
struct ed_stream_core_opts { int chunk_frames, filter, fsm; double filter_alpha, true_threshold; };

/* create: the option checks that need no network, before the owner allocates; then, on a zeroed core for geometry g with F frames per
 * window and n_mics microphones: the fields, hipSetDevice, the HIP stream, the event, every buffer (`front_bytes` of the owner's outputs
 * lead the block) and a reset. free waits for the stream's work and frees whatever create got, also after it failed. */
int ed_stream_core_check_opts(edison_ctx *ctx, const char *who, const edison_kws_geom *g, const ed_stream_core_opts *o);
int ed_stream_core_create(ed_stream_core *c, edison_ctx *ctx, const char *who, int feat_elem, int out_elem, const edison_kws_geom *g, int F,
                          int n_out, int n_mics, const ed_stream_core_opts *o, size_t front_bytes);
void ed_stream_core_free(ed_stream_core *c);

/* A push of n frames on q (host = 1: host samples, q = c->own; host = 0: device samples, q = the context's stream):
 *   begin_push   waits for work left on another HIP stream, shifts the history when the push would not fit, uploads the samples to
 *                d_audio + pos * hop + tail of every microphone (the host's through h_in); the owner's feature rows and network follow
 *   finish_push  where the stream has a filter: the filter (+ edisonFSM) over fin[n][n_mics][n_out] (int8 for out_elem 1, float for 4,
 *                with one microphone or more) into the block; pos += n; host: one download of the block to h_out and one wait; what the getters need to know of this push */
int ed_stream_core_begin_push(ed_stream_core *c, hipStream_t q, const int16_t *samples, int n, int host);
int ed_stream_core_finish_push(ed_stream_core *c, hipStream_t q, const void *fin, int n, int host);
/* finish_push for a push that carries a mask: present [n_mics], nonzero = this microphone's samples count (host = 1: host memory,
 * uploaded through h_present; host = 0: device memory, read on q). out0 / out1 [n][n_mics][n_out] of out_elem bytes and argmax
 * [n][n_mics] are where the owner's network wrote this push (NULL: nowhere). Runs the hold, then finish_push's filter with the mask -- a
 * present microphone as there; an absent one gets zero bytes in its rows of filt, -1 in likely and spotted, its machine's unchanged
 * state in states and the unchanged machine in the copy, and keeps its filter state and its machine -- then what finish_push does
 * behind its filter. */
int ed_stream_core_finish_push_present(ed_stream_core *c, hipStream_t q, const void *fin, int n, int host, const unsigned char *present, void *out0,
                                       void *out1, int32_t *argmax);

/* c = NULL: EDISON_E_ARGUMENT. The getters copy the last push's outputs (host = 1: host pointers, synchronous; host = 0: device
 * pointers, ordered on the context's stream; NULL: not copied); fsm [n_mics]. */
int ed_stream_core_reset(ed_stream_core *c);
/* microphone `mic` alone back to a new stream's state, at the current pos: history, filter state, state machine. Waits for pushes left
 * on another HIP stream and returns when it is done, as reset. */
int ed_stream_core_reset_mic(ed_stream_core *c, int mic);
/* counts [n_mics] (host): the frames each microphone was present for since create or reset, frames_seen minus what it missed. Waits for
 * pushes left on another HIP stream and returns when it is done, as reset_mic. NULL: EDISON_E_ARGUMENT. */
int ed_stream_core_frames_seen_mics(ed_stream_core *c, int64_t *counts);
int ed_stream_core_filtered(ed_stream_core *c, float *filt, int32_t *likely, int32_t *spotted, int host);
int ed_stream_core_fsm(ed_stream_core *c, edison_fsm *fsm, int32_t *states, int host);

#endif
