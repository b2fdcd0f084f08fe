/*
 * edison_stream_geom.h -- what edison_stream_geom.hip (one microphone) and edison_stream_bank.hip (many) share around the sliding-window
 * core: both run the int8 graph loaded on the context behind the float64 MFCC of one geometry. Defined in edison_stream_geom.hip. Not
 * part of the public ABI.
 */
#ifndef EDISON_STREAM_GEOM_H
#define EDISON_STREAM_GEOM_H

#include "edison_stream_core.h"
#include "mfcc_geom.h"

/* the features and the graph of one stream or bank */
struct ed_stream_geom_part
{
	int has_softmax;
	ed_geom_cache tab;             /* tables of its own (edison_kws_geom.hip builds them) */
	ed_geom_args_t margs;          /* tab.tmpl with the per-geometry fields; audio, feat and the frame counts are set per push */
	int model_epoch;
};

/* every check of edison_stream_geom_create behind the NULL checks, messages led by `who`; *F = frames per window, *co = the core's options */
int ed_stream_geom_check_create(edison_ctx *ctx, const char *who, const edison_kws_geom *g, const edison_stream_geom_opts *o, int *F,
                                ed_stream_core_opts *co);
/* the tables and the MFCC launch template for g, the graph's softmax flag and the model's epoch; free releases the tables */
int ed_stream_geom_part_init(edison_ctx *ctx, const edison_kws_geom *g, ed_stream_geom_part *p);
void ed_stream_geom_part_free(ed_stream_geom_part *p);
/* EDISON_E_ARGUMENT with a message led by `who` when the model was reloaded after init */
int ed_stream_geom_part_check(edison_ctx *ctx, const char *who, const ed_stream_geom_part *p);
/* the network on the kernel edison_net_batch_dev picks for the loaded graph, on hipStream q: n inputs, `stride` bytes apart */
int ed_stream_geom_net_on(edison_ctx *ctx, hipStream_t q, const int8_t *in, int n, int64_t stride, int8_t *logits, int8_t *softmax, int32_t *argmax);

#endif
