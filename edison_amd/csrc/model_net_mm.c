/*
 * model_net_mm.c -- host-side planner of the matrix-core path for ANY sequential NNoM int8 graph (the layer list
 * ed_plan_net built): operand-fragment packing of every Conv2D / Dense layer, the padded activation layouts and the
 * LDS budget. The arithmetic it feeds is the reference's (arm_convolve_HWC_q7_basic_nonsquare.c:188-221,
 * arm_fully_connected_q7_opt.c:374-473: out = sat8((sum x*w + (bias << BL) + NN_ROUND(RS)) >> RS)); only the order of
 * the exact integer sums differs. See edison_internal.h (ed_mm_plan_t) for the scheme.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/edison_hip.h"
#include "edison_internal.h"

typedef struct { int32_t v[12]; } rec_t;

static int imax(int a, int b) { return a > b ? a : b; }
static int up16(int v) { return (v + 15) & ~15; }

int ed_plan_net_mm(const void *blob, size_t blob_bytes, const ed_net_plan_t *plan, ed_mm_plan_t *mm, int8_t **frag, int32_t **seeds)
{
	const unsigned char *p = (const unsigned char *)blob;
	memset(mm, 0, sizeof(*mm));
	*frag = NULL;
	*seeds = NULL;
	if (blob_bytes < 40) return EDISON_E_SIZE;
	const int n_layers = plan->n_layers;
	/* A branching graph (a source table: Add, Sub, Mult, Concat, hooks from earlier layers): who reads each tensor. A sequential
	 * graph takes none of the branches below that test `br`, so its plan is what it always was. */
	const int br = plan->branching;
#define SRC_N(j) (plan->src[plan->L[j].src_off])
#define SRC(j, k) (plan->src[plan->L[j].src_off + 1 + (k)])
	int nread[ED_NET_MAX_LAYERS], only[ED_NET_MAX_LAYERS], lastr[ED_NET_MAX_LAYERS]; /* reads of tensor t, its reader if there is one only, its last reader */
	int cons[ED_NET_MAX_LAYERS];  /* the reader in whose LDS layout tensor t is stored; n_layers: compact */
	int held[ED_NET_MAX_LAYERS];  /* 1: tensor t lives in a held area, not in the ping-pong region */
	int hoff[ED_NET_MAX_LAYERS], timg[ED_NET_MAX_LAYERS], loc[ED_NET_MAX_LAYERS + 1]; /* held offset (per input), bytes per image, place in the slice */
	int spass[ED_NET_MAX_LAYERS]; /* the pass that stores tensor t: t itself, or t - 1 for the output of a MaxPool fused into the convolution in front */
	int hold_img = 0, n_msrc = 0;
	loc[0] = 0;
	for (int t = 0; t < n_layers; t++) { nread[t] = 0; only[t] = -1; lastr[t] = t; cons[t] = t + 1 < n_layers ? t + 1 : n_layers; spass[t] = t; held[t] = 0; hoff[t] = 0; timg[t] = 0; }
	for (int j = 0; j < n_layers && br; j++)
		for (int k = 0; k < SRC_N(j); k++)
		{
			const int t = SRC(j, k);
			if (t < 0) { if (j != 0 || SRC_N(j) != 1) return EDISON_OK; continue; } /* the network input: layer 0 alone reads it on this path */
			only[t] = nread[t] == 0 || only[t] == j ? j : -2;
			nread[t]++;
			lastr[t] = j;
		}
	if (br && SRC(0, 0) != -1) return EDISON_OK;
	const int8_t *payload = (const int8_t *)(p + 40 + (size_t)n_layers * 48);

	/* pass 1: shapes, counts */
	size_t frag_bytes = 0;
	int n_seeds = 0, n_koff = 0;
	for (int i = 0; i < n_layers; i++)
	{
		const ed_net_layer_t *L = &plan->L[i];
		ed_mm_layer_t *M = &mm->L[i];
		/* default: the layer reads a compact (unpadded) image */
		M->in_hp = L->in_h; M->in_wp = L->in_w; M->in_py = 0; M->in_px = 0;
		M->pp = L->type == ED_NET_DENSE ? L->in_n : L->in_c;
		/* (a dense layer reads the same compact HWC image: it is a 1x1 convolution over ONE row of in_n bytes) */
		if (L->type != ED_NET_CONV && L->type != ED_NET_DENSE)
		{
			M->in_img = up16(L->in_n) + 16;
			if (L->type == ED_NET_DWCONV)
			{
				/* VALU layer inside the launch (ED_RUN_DW): its weights travel with the fragments, one dword per (tap, group of four
				 * channels), its seeds with the seeds, four per group (both zero beyond C: a group's spare lanes compute nothing stored) */
				const int c4n = (L->in_c + 3) / 4;
				M->frag_off = (int32_t)frag_bytes;
				frag_bytes += (size_t)up16(4 * c4n * L->kh * L->kw);
				M->seed_off = n_seeds;
				n_seeds += 4 * c4n;
			}
			continue;
		}
		const int dense = L->type == ED_NET_DENSE;
		const int in_c = dense ? L->in_n : L->in_c, kh = dense ? 1 : L->kh, kw = dense ? 1 : L->kw;
		const int sh = dense ? 1 : L->sh, out_w = dense ? 1 : L->out_w, out_h = dense ? 1 : L->out_h;
		if (!dense)
		{
			/* zero border so that every window lies inside the stored image: pad rows / columns in front
			 * (nnom_conv2d.c:66-71) and whatever the last windows overhang behind */
			M->in_py = L->pad_h; M->in_px = L->pad_w;
			M->in_hp = imax(L->in_h + L->pad_h, (out_h - 1) * L->sh + kh);
			M->in_wp = imax(L->in_w + L->pad_w, (out_w - 1) * L->sw + kw);
		}
		const int seg = kw * in_c;                 /* contiguous bytes under one kernel row */
		M->mm = 1;
		M->cpr = (seg + 15) / 16;
		M->n_ks = (kh * M->cpr + 1) / 2;
		M->n_rt = (L->out_c + 31) / 32;
		M->expand = (in_c % 16) != 0;
		/* Row-Toeplitz form of a convolution over a NARROW image with few channels (a spectrogram: C_in = 1): the GEMM's rows
		 * are (output x, output channel) pairs, its k runs over (kernel row, byte of the WHOLE zero-padded input row, 16-byte
		 * aligned by construction), its columns are the output rows. A[(x, oc)][ky][q] = w[oc][ky][q / C_in - x * sw][q % C_in]
		 * where that tap exists, else 0. No expanded copy of the input (the expansion pass and its LDS buffer -- 4.4 KB per
		 * input on kws_conv, more than both activation buffers together -- disappear), and the output row of a column is
		 * contiguous in the consumer's HWC layout, so the epilogue is the ordinary one with out_w * C_out "channels".
		 * Taken when the plain form would need the expansion, the padded row fits four chunks and the matrix-core work does
		 * not grow by more than half. EDISON_NET_NO_TOEPLITZ=1: A/B knob. */
		if (!dense && M->expand)
		{
			const char *env = getenv("EDISON_NET_NO_TOEPLITZ");
			const int rowb = up16(M->in_wp * in_c), rows = L->out_w * L->out_c;
			const int64_t plain = (int64_t)M->n_rt * ((out_h * out_w + 31) / 32) * M->n_ks;
			const int64_t toep = (int64_t)((rows + 31) / 32) * ((out_h + 31) / 32) * ((kh * (rowb / 16) + 1) / 2);
			if (!(env && atoi(env)) && rowb <= 64 && rowb % in_c == 0 && rows <= 1024 && 2 * toep <= 3 * plain)
			{
				M->toep = 1;
				M->in_wp = rowb / in_c;               /* zero columns behind the image up to the aligned row */
				M->cpr = rowb / 16;
				M->n_ks = (kh * M->cpr + 1) / 2;
				M->n_rt = (rows + 31) / 32;
				M->expand = 0;
			}
		}
		M->in_img = (dense ? up16(L->in_n) : up16(M->in_hp * M->in_wp * in_c)) + 16; /* dense: the compact image, C_in = its whole length */
		if (M->toep)
		{
			M->pitch_x = 0;                           /* one GEMM column per output ROW */
			M->pitch_y = M->in_wp * in_c;
			M->x_img = 0;
		}
		else if (M->expand)
		{
			M->pitch_x = 16 * M->cpr;
			M->pitch_y = out_w * 16 * M->cpr;
			M->x_img = (dense ? 1 : M->in_hp) * M->pitch_y + 16;
		}
		else
		{
			M->pitch_x = (dense ? 1 : L->sw) * in_c;
			M->pitch_y = M->in_wp * in_c;
			M->x_img = 0;
		}
		(void)sh;
		/* the small-tile form of the same layer (chosen in pass 2, once the per-wave batch is known): room for either */
		M->n_ks16 = (kh * M->cpr + 3) / 4;
		M->n_rt16 = ((M->toep ? L->out_w * L->out_c : L->out_c) + 15) / 16;
		M->frag_off = (int32_t)frag_bytes;
		frag_bytes += (size_t)imax(M->n_rt * M->n_ks, M->n_rt16 * M->n_ks16) * 1024;
		M->seed_off = n_seeds;
		n_seeds += 32 * M->n_rt;
		M->koff_off = n_koff;
		n_koff += imax(2 * M->n_ks, 4 * M->n_ks16);
		if (n_koff > ED_MM_MAX_KOFF || 2 * M->n_ks > 256 || frag_bytes > ((size_t)64 << 20)) return EDISON_OK; /* mm->ok stays 0 */
	}

	/* MaxPool right behind a matrix-core layer, window = stride, no padding, at most 4 positions: fused into that layer */
	for (int i = 0; i + 1 < n_layers; i++)
	{
		const ed_net_layer_t *C = &plan->L[i], *Q = &plan->L[i + 1];
		if (!mm->L[i].mm || C->type != ED_NET_CONV || Q->type != ED_NET_POOL) continue;
		if (Q->pad_h || Q->pad_w || Q->check_taps || Q->kh != Q->sh || Q->kw != Q->sw || (Q->kh * Q->kw != 2 && Q->kh * Q->kw != 4)) continue;
		if (Q->out_h * Q->kh > C->out_h || Q->out_w * Q->kw > C->out_w) continue;
		if (mm->L[i].toep && (Q->kw != 1 || Q->out_w != C->out_w)) continue; /* x lives in the GEMM's rows there: only windows along y fuse */
		if (br && !(nread[i] == 1 && only[i] == i + 1 && SRC_N(i + 1) == 1)) continue; /* something else reads the unpooled tensor */
		mm->L[i].pool_h = Q->kh; mm->L[i].pool_w = Q->kw;
		mm->L[i + 1].skip = 1;
		mm->L[i + 1].in_img = 0; /* the unpooled tensor never exists */
		spass[i + 1] = i;        /* the pooled one is stored while pass i still reads its inputs */
	}

	/* LDS banks. A B fragment is 16 bytes per lane and neighbouring lanes are neighbouring pixels; the epilogue of the layer in
	 * front stores one dword per lane, neighbouring lanes again neighbouring pixels. With C_in = 32 or 64 bytes per pixel the 16
	 * lanes of a read phase fall on every second / fourth 16-byte bank group and the stores on 8 / 4 of the 64 banks (the own
	 * kernel of kws_conv: LDS pipe 86 % busy, 43 % of it conflicts, profiles/r03_net_counters.txt). One 16-byte gap behind every
	 * pixel whose C_in is an EVEN multiple of 16 makes the pixel pitch an odd multiple: consecutive pixels then walk through all
	 * 16 bank groups. Only the tables change (chunk offsets, column offsets, the producer's output pitch); the gaps are never
	 * read. Not for layers that read an expanded copy or a Toeplitz row, not behind a Toeplitz producer (it stores whole rows),
	 * not for Dense (one column per image: nothing to conflict with). EDISON_NET_NO_PIXEL_GAP=1: A/B knob. */
	{
		const char *env = getenv("EDISON_NET_NO_PIXEL_GAP");
		for (int i = 0; i < n_layers && !(env && atoi(env)) && !br; i++) /* (a branching graph: the producer is not the layer in front) */
		{
			const ed_net_layer_t *L = &plan->L[i];
			ed_mm_layer_t *M = &mm->L[i];
			if (!M->mm || L->type != ED_NET_CONV || M->expand || M->toep || (L->in_c % 32) != 0) continue;
			int j = i - 1; /* the producer: the layer in front, or the one in front of a fused MaxPool */
			if (j >= 0 && mm->L[j].skip) j--;
			if (j >= 0 && mm->L[j].toep) continue;
			if (j < 0 && !(plan->in_n <= ED_MM_MAX_INTAB)) continue; /* the input stage places pixels by table only */
			M->pp = L->in_c + 16;
			M->pitch_x = L->sw * M->pp;
			M->pitch_y = M->in_wp * M->pp;
			M->in_img = up16(M->in_hp * M->in_wp * M->pp) + 16;
		}
	}

	/* A branching graph stores a tensor ONCE, in the layout of the one reader that demands one: a matrix-core convolution wants its zero
	 * border (and reads an expanded copy from there), the pool / DW / AvgPool / Dense / Softmax passes a compact image, the merge passes
	 * read any layout through msrc[]. Two readers that demand different layouts (an inception stem: a 1x1 and a padded 3x3 convolution)
	 * keep the graph on the layer-by-layer kernel. */
	for (int t = 0; t < n_layers && br; t++)
	{
		int first = -1, conv = -1, merge = -1;
		for (int j = t + 1; j < n_layers; j++)
			for (int k = 0; k < SRC_N(j); k++)
			{
				if (SRC(j, k) != t) continue;
				if (ED_NET_IS_MERGE(plan->L[j].type)) { if (merge < 0) merge = j; continue; }
				if (first < 0) first = j;
				if (conv < 0 && plan->L[j].type == ED_NET_CONV) conv = j;
			}
		const int pick = conv >= 0 ? conv : first;
		cons[t] = pick >= 0 ? pick : merge >= 0 ? merge : n_layers;
		for (int j = t + 1; j < n_layers && pick >= 0; j++)
		{
			if (ED_NET_IS_MERGE(plan->L[j].type) || SRC(j, 0) != t || mm->L[j].skip) continue;
			const ed_mm_layer_t *A = &mm->L[pick], *B = &mm->L[j];
			const int pa = plan->L[pick].type == ED_NET_CONV ? A->pp : plan->L[t].out_c, pb = plan->L[j].type == ED_NET_CONV ? B->pp : plan->L[t].out_c;
			if (A->in_hp != B->in_hp || A->in_wp != B->in_wp || A->in_py != B->in_py || A->in_px != B->in_px || A->in_img != B->in_img || pa != pb) return EDISON_OK;
		}
	}
	/* which tensors are held: every one that something else than the very next pass reads (or that is read twice); then a place for
	 * each in the held area by liveness, first fit, in bytes per input (the per-wave batch scales them). Tensor t lives from the pass
	 * that stores it, spass[t], to its last reader, both included: a pass reads its inputs while it stores its output, so an earlier
	 * tensor u is in t's way while lastr[u] >= spass[t] (stored tensors have distinct, increasing spass[]) */
	for (int t = 0; t < n_layers && br; t++)
	{
		if (mm->L[t].pool_h > 0) continue;               /* never stored: its fused MaxPool's output is */
		int next = t + 1;
		while (next < n_layers && mm->L[next].skip) next++;
		held[t] = nread[t] > 0 && !(nread[t] == 1 && only[t] == next);
		timg[t] = cons[t] < n_layers ? mm->L[cons[t]].in_img : up16(plan->L[t].out_n) + 16;
	}
	for (int t = 0; t < n_layers && br; t++)
	{
		if (!held[t]) continue;
		int at = 0, moved = 1;
		while (moved)
		{
			moved = 0;
			for (int u = 0; u < t; u++)
				if (held[u] && lastr[u] >= spass[t] && at < hoff[u] + timg[u] && hoff[u] < at + timg[t]) { at = hoff[u] + timg[u]; moved = 1; }
		}
		hoff[t] = at;
		if (at + timg[t] > hold_img) hold_img = at + timg[t];
	}

	/* column tables: (B offset, output offset) of every stored pixel, for the layers that fit ED_MM_MAX_COLS together */
	int n_cols = 0;
	for (int i = 0; i < n_layers; i++)
	{
		const ed_net_layer_t *L = &plan->L[i];
		ed_mm_layer_t *M = &mm->L[i];
		M->col_off = -1;
		if (!M->mm) continue;
		const int dense = L->type == ED_NET_DENSE, fused = M->pool_h > 0, nx = cons[fused ? i + 1 : i];
		const int st_h = dense ? 1 : (fused ? plan->L[i + 1].out_h : L->out_h), st_w = dense || M->toep ? 1 : (fused ? plan->L[i + 1].out_w : L->out_w);
		if (n_cols + st_h * st_w > ED_MM_MAX_COLS) continue;
		const int ph = fused ? M->pool_h : 1, pw = fused ? M->pool_w : 1, sh = dense ? 1 : L->sh;
		int owp, opy, opx, opp; /* the consumer's layout (the last layer's output is compact) */
		if (nx < n_layers) { owp = mm->L[nx].in_wp; opy = mm->L[nx].in_py; opx = mm->L[nx].in_px; opp = plan->L[nx].type == ED_NET_CONV ? mm->L[nx].pp : L->out_c; }
		else { owp = fused ? plan->L[i + 1].out_w : L->out_w; opy = 0; opx = 0; opp = L->out_c; }
		M->col_off = n_cols;
		for (int y = 0; y < st_h; y++)
			for (int x = 0; x < st_w; x++)
			{
				mm->coltab[2 * n_cols] = (y * ph * sh) * M->pitch_y + (x * pw) * M->pitch_x;
				mm->coltab[2 * n_cols + 1] = ((y + opy) * owp + x + opx) * opp;
				n_cols++;
			}
	}
	mm->n_cols = n_cols;

	/* expansion tables and the input table, under the same rule (what does not fit is worked out by the kernel) */
	int n_xtab = 0;
	for (int i = 0; i < n_layers; i++)
	{
		const ed_net_layer_t *L = &plan->L[i];
		ed_mm_layer_t *M = &mm->L[i];
		M->xtab_off = -1;
		if (!M->mm || !M->expand) continue;
		const int dense = L->type == ED_NET_DENSE;
		const int in_c = dense ? L->in_n : L->in_c, seg = (dense ? 1 : L->kw) * in_c, sw = dense ? 1 : L->sw, out_w = dense ? 1 : L->out_w;
		const int rows = dense ? 1 : M->in_hp, rec = rows * out_w * M->cpr;
		if (n_xtab + rec > ED_MM_MAX_XTAB || M->in_img >= (1 << 24)) continue;
		M->xtab_off = n_xtab;
		for (int r = 0; r < rows; r++)
			for (int xo = 0; xo < out_w; xo++)
				for (int j = 0; j < M->cpr; j++)
				{
					const int keep = seg - 16 * j < 16 ? seg - 16 * j : 16;
					mm->xtab[2 * n_xtab] = ((r * M->in_wp + xo * sw) * in_c + 16 * j) | (keep << 24);
					mm->xtab[2 * n_xtab + 1] = r * M->pitch_y + xo * M->pitch_x + 16 * j;
					n_xtab++;
				}
	}
	mm->n_xtab = n_xtab;
	mm->n_intab = 0;
	if (plan->in_n <= ED_MM_MAX_INTAB && mm->L[0].in_img <= 65536)
	{
		const ed_mm_layer_t *M0 = &mm->L[0];
		for (int e = 0; e < plan->in_n; e++)
		{
			const int pix = e / plan->in_c, c = e - pix * plan->in_c, y = pix / plan->in_w, x = pix - y * plan->in_w;
			mm->intab[e] = (uint16_t)(((y + M0->in_py) * M0->in_wp + x + M0->in_px) * (plan->L[0].type == ED_NET_CONV ? M0->pp : plan->in_c) + c);
		}
		mm->n_intab = plan->in_n;
		if (plan->in_n >= 4 && plan->in_n < ED_MM_INTAB_PAD) /* see ED_MM_INTAB_PAD */
		{
			for (int e = plan->in_n; e < ED_MM_INTAB_PAD; e++) mm->intab[e] = (uint16_t)(M0->in_img - 1);
			mm->n_intab = ED_MM_INTAB_PAD;
		}
	}

	/* LDS budget: a wave's activation region for `batch` inputs -- a layer's input images at one end, its output images at
	 * the other, the next layer the other way round: max(in + out) over the layers that run, not twice the largest image --
	 * the expansion buffer, the koff table */
	int max_pair = 0, max_x = 0;
	for (int i = 0; i < n_layers; i++)
	{
		if (mm->L[i].x_img > max_x) max_x = mm->L[i].x_img;
		if (mm->L[i].skip) continue;
		const int nx = cons[mm->L[i].pool_h > 0 ? i + 1 : i];
		const int st_h = mm->L[i].pool_h > 0 ? plan->L[i + 1].out_h : plan->L[i].out_h, st_w = mm->L[i].pool_h > 0 ? plan->L[i + 1].out_w : plan->L[i].out_w;
		const int out_img = nx < n_layers ? mm->L[nx].in_img : up16(st_h * st_w * plan->L[i].out_c) + 16; /* the last layer's output is compact */
		if (br)
		{
			/* of a pass's inputs at most one is in the region (the pass in front stored it there), the others are held; so may its output be */
			int in_sz = i == 0 ? mm->L[0].in_img : 0;
			for (int k = 0; k < SRC_N(i); k++)
				if (SRC(i, k) >= 0 && !held[SRC(i, k)]) in_sz = timg[SRC(i, k)];
			const int pair = in_sz + (held[mm->L[i].pool_h > 0 ? i + 1 : i] ? 0 : out_img);
			if (pair > max_pair) max_pair = pair;
			continue;
		}
		if (mm->L[i].in_img + out_img > max_pair) max_pair = mm->L[i].in_img + out_img;
	}
	const int max_img = (max_pair / 2 + 15) & ~15; /* half of the region per input */
	/* Where the weight fragments live: (2) ALL layers resident in LDS for the whole launch, shared by the waves of the
	 * workgroup (one L2 read per workgroup), or (0) streamed from L2 per MFMA. Every wave gets its own activation slice
	 * (two ping-pong buffers + the expansion buffer for `batch` inputs); as many waves as fit, at most 12, at least 4; the
	 * per-wave batch grows (up to 4) only while 8 waves still fit -- independent waves hide each other's latencies, a
	 * bigger batch only fills the 32-column tiles of small late layers better. */
	const int lds_cap = 156 * 1024; /* of the CU's 160 KB */
	const int tbl = up16(4 * n_koff) + up16(4 * n_seeds) + up16(8 * n_cols) + up16(8 * n_xtab) + up16(2 * mm->n_intab);
	if (tbl > 24 * 1024) return EDISON_OK;
	int batch = 0, waves = 0, frag_lds = 0, frag_mode = 0;
	/* EDISON_NET_BATCH=b / EDISON_NET_MIN_WAVES=w: A/B knobs (tools/bench_net.py): force the per-wave batch, relax the wave floor */
	const char *env_b = getenv("EDISON_NET_BATCH"), *env_w = getenv("EDISON_NET_MIN_WAVES");
	const int force_b = env_b ? atoi(env_b) : 0, min_w = env_w ? atoi(env_w) : 0;
	for (int mode = 2; mode >= 0 && !batch; mode -= 2)
	{
		const int64_t fl = mode == 2 ? (int64_t)frag_bytes : 0;
		if (fl > 96 * 1024) continue;
		for (int b = 4; b >= 1 && !batch; b >>= 1)
		{
			if (force_b > 0 && b != force_b) continue;
			const int64_t per_wave = 2 * (int64_t)b * max_img + (int64_t)b * up16(max_x) + (int64_t)b * hold_img;
			int64_t w = (lds_cap - tbl - fl) / per_wave;
			if (w > 12) w = 12; /* the kernel is built for 768 threads: 168 VGPRs a wave */
			if (w >= (min_w > 0 ? min_w : (b > 1 ? 8 : 4))) { batch = b; waves = (int)w; frag_lds = (int)fl; frag_mode = mode; }
		}
	}
	if (!batch) return EDISON_OK;
	mm->batch = batch;
	mm->waves = waves;
	mm->buf_bytes = batch * max_img;
	mm->x_bytes = batch * up16(max_x);
	mm->hold_bytes = batch * hold_img;
	mm->frag_lds = frag_lds;
	mm->frag_mode = frag_mode;
	mm->tbl_bytes = tbl;
	mm->lds_bytes = tbl + frag_lds + waves * (2 * mm->buf_bytes + mm->x_bytes + mm->hold_bytes);
	mm->frag_bytes = (int32_t)frag_bytes;
	mm->n_seeds = n_seeds;
	mm->n_koff = n_koff;

	/* layers whose columns (stored pixels x per-wave batch) fit 16 and that fuse no MaxPool run on 16 x 16 x 64 tiles: a
	 * quarter of the accumulator registers to requantise per tile and half the k-steps, where a 32-column tile would be
	 * mostly padding (the late layers of a classifier: 3 pixels, 1 pixel). EDISON_NET_NO_SMALL_TILES=1: A/B knob. */
	{
		const char *env = getenv("EDISON_NET_NO_SMALL_TILES");
		const int no_small = env && atoi(env);
		for (int i = 0; i < n_layers; i++)
		{
			const ed_net_layer_t *L = &plan->L[i];
			ed_mm_layer_t *M = &mm->L[i];
			if (!M->mm) continue;
			const int dense = L->type == ED_NET_DENSE;
			const int pix = dense ? 1 : L->out_h * (M->toep ? 1 : L->out_w);
			M->small = !no_small && M->pool_h == 0 && batch * pix <= 16;
		}
		/* now that every layer's form is known: the exact fragment layout (pass 1 reserved room for either form), and
		 * the waves that fit beside it */
		size_t fexact = 0;
		for (int i = 0; i < n_layers; i++)
		{
			ed_mm_layer_t *M = &mm->L[i];
			if (plan->L[i].type == ED_NET_DWCONV)
			{
				M->frag_off = (int32_t)fexact;
				fexact += (size_t)up16(4 * ((plan->L[i].in_c + 3) / 4) * plan->L[i].kh * plan->L[i].kw);
				continue;
			}
			if (!M->mm) continue;
			M->frag_off = (int32_t)fexact;
			fexact += (size_t)(M->small ? M->n_rt16 * M->n_ks16 : M->n_rt * M->n_ks) * 1024;
		}
		frag_bytes = fexact;
		if (frag_mode == 2) frag_lds = (int)fexact;
		{
			const int64_t per_wave = 2 * (int64_t)batch * max_img + (int64_t)batch * up16(max_x) + (int64_t)batch * hold_img;
			int64_t w = (lds_cap - tbl - frag_lds) / per_wave;
			if (w > 12) w = 12;
			if (w > waves) waves = (int)w;
		}
		mm->waves = waves;
		mm->frag_lds = frag_lds;
		mm->lds_bytes = tbl + frag_lds + waves * (2 * mm->buf_bytes + mm->x_bytes + mm->hold_bytes);
		mm->frag_bytes = (int32_t)frag_bytes;
	}

	/* pass 2: fragments, seeds, chunk offsets */
	int8_t *fb = (int8_t *)calloc(frag_bytes + 16, 1);
	int32_t *sb = (int32_t *)calloc((size_t)n_seeds + 4, sizeof(int32_t));
	if (!fb || !sb) { free(fb); free(sb); return EDISON_E_NO_MEMORY; }
	int64_t acc_bound[ED_NET_MAX_LAYERS]; /* the largest |accumulator| a layer can reach, for the choice of its requantisation (ED_RUN_RS_HI) */
	memset(acc_bound, 0, sizeof(acc_bound));
	for (int i = 0; i < n_layers; i++)
	{
		const ed_net_layer_t *L = &plan->L[i];
		const ed_mm_layer_t *M = &mm->L[i];
		if (L->type == ED_NET_DWCONV)
		{
			rec_t r;
			memcpy(&r, p + 40 + (size_t)i * 48, sizeof(r));
			const int c = L->in_c, c4n = (c + 3) / 4;
			const int8_t *w = payload + r.v[9], *bias = payload + r.v[10]; /* [ky][kx][ch] */
			for (int t = 0; t < L->kh * L->kw; t++)
				for (int ch = 0; ch < c; ch++) fb[M->frag_off + (size_t)4 * c4n * t + ch] = w[(size_t)t * c + ch];
			for (int ch = 0; ch < c; ch++)
				sb[M->seed_off + ch] = (int32_t)((uint32_t)(int32_t)bias[ch] << r.v[6]) + (int32_t)((1u << r.v[7]) >> 1);
			continue;
		}
		if (!M->mm) continue;
		rec_t r;
		memcpy(&r, p + 40 + (size_t)i * 48, sizeof(r));
		const int dense = L->type == ED_NET_DENSE;
		const int in_c = dense ? L->in_n : L->in_c, kh = dense ? 1 : L->kh, kw = dense ? 1 : L->kw;
		const int8_t *w = payload + r.v[9], *bias = payload + r.v[10]; /* OHWI / [out][in]: row o = kh segments of seg bytes */
		int8_t *wt = NULL;
		int seg = kw * in_c, n_rows = L->out_c;
		for (int o = 0; o < L->out_c; o++) /* |sum x w + seed| <= 128 sum |w| + |seed| */
		{
			int64_t sw = 0;
			for (int q = 0; q < kh * seg; q++) sw += w[(size_t)o * kh * seg + q] < 0 ? -(int64_t)w[(size_t)o * kh * seg + q] : w[(size_t)o * kh * seg + q];
			const int64_t sd = (int64_t)(int32_t)((uint32_t)(int32_t)bias[o] << r.v[6]) + (int64_t)((1u << r.v[7]) >> 1);
			const int64_t bd = 128 * sw + (sd < 0 ? -sd : sd);
			if (bd > acc_bound[i]) acc_bound[i] = bd;
		}
		if (M->toep)
		{
			/* the Toeplitz matrix, in the layout the packing below expects: [row = x * C_out + oc][ky][q < rowb] */
			const int rowb = M->in_wp * in_c;
			n_rows = L->out_w * L->out_c;
			wt = (int8_t *)calloc((size_t)n_rows * kh * rowb, 1);
			if (!wt) { free(fb); free(sb); return EDISON_E_NO_MEMORY; }
			for (int x = 0; x < L->out_w; x++)
				for (int o = 0; o < L->out_c; o++)
					for (int ky = 0; ky < kh; ky++)
						for (int t = 0; t < kw; t++)
							for (int c = 0; c < in_c; c++)
								wt[(((size_t)x * L->out_c + o) * kh + ky) * rowb + (x * L->sw + t) * in_c + c] = w[((size_t)o * kh + ky) * seg + t * in_c + c];
			w = wt;
			seg = rowb;
		}
		if (M->small)
		{
			/* lane l of k-step s of row tile rt: row 16 rt + (l & 15), chunk 4 s + (l >> 4) */
			for (int rt = 0; rt < M->n_rt16; rt++)
				for (int s = 0; s < M->n_ks16; s++)
				{
					int8_t *f = fb + M->frag_off + ((size_t)rt * M->n_ks16 + s) * 1024;
					for (int l = 0; l < 64; l++)
					{
						const int row = 16 * rt + (l & 15), c = 4 * s + (l >> 4);
						const int ky = c / M->cpr, jc = c - ky * M->cpr;
						for (int j = 0; j < 16; j++)
						{
							const int q = 16 * jc + j;
							f[l * 16 + j] = (row < n_rows && ky < kh && q < seg) ? w[((size_t)row * kh + ky) * seg + q] : 0;
						}
					}
				}
		}
		else
		for (int rt = 0; rt < M->n_rt; rt++)
			for (int s = 0; s < M->n_ks; s++)
			{
				int8_t *f = fb + M->frag_off + ((size_t)rt * M->n_ks + s) * 1024;
				for (int l = 0; l < 64; l++)
				{
					const int row = 32 * rt + (l & 31), c = 2 * s + (l >> 5);
					const int ky = c / M->cpr, jc = c - ky * M->cpr;
					for (int j = 0; j < 16; j++)
					{
						const int q = 16 * jc + j;
						f[l * 16 + j] = (row < n_rows && ky < kh && q < seg) ? w[((size_t)row * kh + ky) * seg + q] : 0;
					}
				}
			}
		free(wt);
		for (int o = 0; o < n_rows; o++)
			sb[M->seed_off + o] = (int32_t)((uint32_t)(int32_t)bias[o % L->out_c] << r.v[6]) + (int32_t)((1u << r.v[7]) >> 1);
		for (int c = 0; c < (M->small ? 4 * M->n_ks16 : 2 * M->n_ks); c++)
		{
			const int ky = c / M->cpr, jc = c - ky * M->cpr;
			/* chunk jc of a kernel row: 16 bytes of pixel jc / (C_in / 16) -- behind a pixel gap the row is not contiguous */
			const int in_row = (!dense && M->pp != in_c) ? (jc / (in_c / 16)) * M->pp + (jc % (in_c / 16)) * 16 : 16 * jc;
			mm->koff[M->koff_off + c] = ky < kh ? ky * M->pitch_y + in_row : 0; /* chunks past the end meet zero weights */
		}
	}
	/* bounds of everything the kernel will address in LDS, checked here on the host (a plan that fails stays off the
	 * matrix-core path instead of reaching the device): B fragment reads and epilogue stores of every layer */
	int in_off = 0; /* the first layer's input sits at the low end of the region */
	const int region = 2 * mm->buf_bytes;
	for (int i = 0; i < n_layers; i++)
	{
		const ed_net_layer_t *L = &plan->L[i];
		const ed_mm_layer_t *M = &mm->L[i];
		if (M->skip) continue; /* fused MaxPool: nothing runs for it */
		int ohp, owp, opy, opx, oimg, opp; /* the consumer's layout = where this layer's epilogue stores */
		const int fused = M->pool_h > 0, st = fused ? i + 1 : i, nx = cons[st]; /* the tensor this pass stores; the reader whose layout it gets */
		const int st_h = fused ? plan->L[i + 1].out_h : L->out_h, st_w = fused ? plan->L[i + 1].out_w : L->out_w; /* what is stored */
		if (nx < n_layers) { ohp = mm->L[nx].in_hp; owp = mm->L[nx].in_wp; opy = mm->L[nx].in_py; opx = mm->L[nx].in_px; oimg = mm->L[nx].in_img; opp = plan->L[nx].type == ED_NET_CONV ? mm->L[nx].pp : L->out_c; }
		else { ohp = st_h; owp = st_w; opy = 0; opx = 0; oimg = up16(st_h * st_w * L->out_c) + 16; opp = L->out_c; }
		const int64_t last_store = ((int64_t)(st_h - 1 + opy) * owp + (st_w - 1 + opx)) * opp + L->out_c;
		/* input at one end of the region, output at the other */
		const int hold0 = region + mm->x_bytes; /* the held areas lie behind the expansion buffer */
		const int o_off = held[st] ? hold0 + batch * hoff[st] : in_off == 0 ? region - batch * oimg : 0;
		int bad = last_store > oimg || ohp < st_h + opy || owp < st_w + opx || o_off < 0 || (o_off & 15) || (in_off & 15);
		int pin = in_off; /* where this pass reads its (first) input */
		if (!br)
		{
			bad |= batch * (M->in_img + oimg) > region;
			bad |= in_off + batch * M->in_img > region || (in_off == 0 ? batch * M->in_img > o_off : batch * oimg > in_off);
		}
		else
		{
			/* every input where the pass that stored it left it; the one that lies in the region must not meet the output there */
			pin = loc[SRC(i, 0) + 1];
			bad |= held[st] ? (oimg != timg[st] || batch * (hoff[st] + oimg) > mm->hold_bytes) : batch * oimg > region;
			for (int k = 0; k < SRC_N(i); k++)
			{
				const int t = SRC(i, k), at = loc[t + 1], sz = batch * (t < 0 ? M->in_img : timg[t]);
				if (t >= 0 && held[t]) { bad |= at < hold0 || at + sz > hold0 + mm->hold_bytes; continue; }
				bad |= at != in_off || at + sz > region; /* the region holds the tensor stored last, nothing older */
				if (!held[st]) bad |= at == 0 ? sz > o_off : batch * oimg > at;
			}
			bad |= !ED_NET_IS_MERGE(L->type) && SRC(i, 0) >= 0 && timg[SRC(i, 0)] != M->in_img;
			/* the output against everything it could destroy, whatever placed the two: every input of this pass wherever it lies, and
			 * every held tensor stored earlier that this pass or a later one still reads */
			for (int k = 0; k < SRC_N(i); k++)
			{
				const int t = SRC(i, k), at = loc[t + 1], sz = batch * (t < 0 ? M->in_img : timg[t]);
				bad |= at < o_off + batch * oimg && o_off < at + sz;
			}
			for (int u = 0; u < st && held[st]; u++)
				if (held[u] && spass[u] < i && lastr[u] >= i)
					bad |= loc[u + 1] < o_off + batch * oimg && o_off < loc[u + 1] + batch * timg[u];
		}
		loc[st + 1] = o_off;
		if (i == 0) loc[0] = 0;
		if (M->mm)
		{
			const int dense = L->type == ED_NET_DENSE;
			const int out_h = dense ? 1 : L->out_h, out_w = dense || M->toep ? 1 : L->out_w, sh = dense ? 1 : L->sh;
			const int img = M->expand ? M->x_img : M->in_img;
			int max_koff = 0;
			for (int c = 0; c < (M->small ? 4 * M->n_ks16 : 2 * M->n_ks); c++) if (mm->koff[M->koff_off + c] > max_koff) max_koff = mm->koff[M->koff_off + c];
			const int64_t last_read = (int64_t)(out_h - 1) * sh * M->pitch_y + (int64_t)(out_w - 1) * M->pitch_x + max_koff + 16;
			bad |= last_read > img || (M->pitch_x & 15) || (M->pitch_y & 15) || (M->in_img & 15) || (M->x_img & 15);
			bad |= M->expand ? (batch * up16(M->x_img) > mm->x_bytes + 0) : 0;
			/* the tables the kernel follows blindly: every entry re-checked against the buffers it indexes */
			if (M->col_off >= 0)
			{
				const int pix = dense ? 1 : st_h * (M->toep ? 1 : st_w), wmax = fused ? ((M->pool_h - 1) * sh) * M->pitch_y + (M->pool_w - 1) * M->pitch_x : 0;
				for (int q = 0; q < pix; q++)
				{
					const int boff = mm->coltab[2 * (M->col_off + q)], ooff = mm->coltab[2 * (M->col_off + q) + 1];
					bad |= boff < 0 || (boff & 15) || (int64_t)boff + wmax + max_koff + 16 > img || ooff < 0 || ooff + (M->toep ? L->out_w : 1) * L->out_c > oimg;
				}
			}
			if (M->xtab_off >= 0)
			{
				const int rec = (dense ? 1 : M->in_hp) * out_w * M->cpr;
				for (int q = 0; q < rec; q++)
				{
					const int w0 = mm->xtab[2 * (M->xtab_off + q)], doff = mm->xtab[2 * (M->xtab_off + q) + 1];
					const int soff = w0 & 0xffffff, keep = w0 >> 24;
					/* the gather reads five aligned dwords around soff: up to soff + 20 */
					bad |= keep < 1 || keep > 16 || soff + 20 > M->in_img + 4 || doff < 0 || (doff & 15) || doff + 16 > M->x_img;
				}
			}
		}
		if (i == 0)
			for (int e = 0; e < mm->n_intab; e++) bad |= mm->intab[e] >= M->in_img;
		bad |= M->toep && opp != L->out_c; /* a Toeplitz layer stores whole rows: its consumer's pixels must be gap-free */
		if (bad) { free(fb); free(sb); return EDISON_OK; } /* mm->ok stays 0 */
		/* the run record */
		ed_mm_run_t *R = &mm->R[i];
		const int dense = L->type == ED_NET_DENSE;
		R->kind = M->mm ? ED_RUN_MM : L->type == ED_NET_POOL ? ((L->in_c & 3) == 0 ? ED_RUN_POOL4 : ED_RUN_POOL1)
		          : L->type == ED_NET_DWCONV ? ED_RUN_DW : L->type == ED_NET_AVGPOOL ? ED_RUN_AVG
		          : L->type == ED_NET_CONCAT ? ED_RUN_CAT : ED_NET_IS_MERGE(L->type) ? ED_RUN_MERGE : ED_RUN_SOFTMAX;
		int msrc0 = 0;
		if (R->kind == ED_RUN_MERGE || R->kind == ED_RUN_CAT)
		{
			/* one msrc entry per input: where its images start in the slice, and the layout its own reader gave it. The merge pass
			 * moves 16-bit words (dwords when C % 4 == 0), like the DW / AvgPool passes: every pitch must keep them aligned */
			if (n_msrc + SRC_N(i) > ED_MM_MAX_MSRC || (R->kind == ED_RUN_MERGE && (L->out_c & 1))) { free(fb); free(sb); return EDISON_OK; }
			const int al = R->kind == ED_RUN_CAT ? 1 : (L->in_c & 3) == 0 ? 4 : 2;
			msrc0 = n_msrc;
			for (int k = 0; k < SRC_N(i); k++)
			{
				const int t = SRC(i, k), cn = t < 0 ? 0 : cons[t];
				if (t < 0) { free(fb); free(sb); return EDISON_OK; }
				int32_t *e = &mm->msrc[5 * n_msrc++];
				const int spp = cn < n_layers ? (plan->L[cn].type == ED_NET_CONV ? mm->L[cn].pp : L->in_c) : L->in_c;
				const int swp = cn < n_layers ? mm->L[cn].in_wp : L->in_w, spy = cn < n_layers ? mm->L[cn].in_py : 0, spx = cn < n_layers ? mm->L[cn].in_px : 0;
				e[0] = loc[t + 1]; e[1] = timg[t]; e[2] = (spy * swp + spx) * spp; e[3] = swp * spp; e[4] = spp;
				const int64_t last_read = (int64_t)e[2] + (int64_t)(L->in_h - 1) * e[3] + (int64_t)(L->in_w - 1) * e[4] + ((L->in_c + al - 1) / al) * al;
				if (last_read > e[1] || (e[2] % al) || (e[3] % al) || (e[4] % al) || (e[0] & 15) || (e[1] & 15)) { free(fb); free(sb); return EDISON_OK; }
			}
		}
		/* the two VALU layers store 16-bit words (dwords when C % 4 == 0) at the consumer's pixel pitch */
		if ((R->kind == ED_RUN_DW || R->kind == ED_RUN_AVG || R->kind == ED_RUN_MERGE) && ((opp & 1) || ((L->in_c & 3) == 0 && (opp & 3)))) { free(fb); free(sb); return EDISON_OK; }
		R->zero_border = ohp != st_h || owp != st_w;
		R->in_img = M->in_img; R->o_img = oimg;
		R->oc_pitch = opp; R->o_origin = (opy * owp + opx) * opp; R->o_row = owp * opp;
		R->li_out = fused ? i + 1 : i;
		R->expand = M->expand; R->x_img = M->x_img; R->xtab_off = M->xtab_off;
		R->rec_per_img = M->mm ? (dense ? 1 : M->in_hp) * (dense ? 1 : L->out_w) * M->cpr : 0;
		R->pitch_x = M->pitch_x; R->pitch_y = M->pitch_y; R->sh = dense ? 1 : L->sh;
		R->ph = fused ? M->pool_h : 1; R->pw = fused ? M->pool_w : 1;
		R->small = M->small;
		R->n_ks = M->small ? M->n_ks16 : M->n_ks; R->n_rt = M->small ? M->n_rt16 : M->n_rt; R->frag_off = M->frag_off; R->seed_off = M->seed_off; R->koff_off = M->koff_off; R->col_off = M->col_off;
		R->pix_per_img = dense ? 1 : st_h * (M->toep ? 1 : st_w); R->col_w = dense || M->toep ? 1 : st_w;
		R->out_c = M->toep ? L->out_w * L->out_c : L->out_c; /* rows of the GEMM */
		R->rs = L->rs; R->lo_clamp = L->relu ? 0 : -128;
		/* sat8(v >> rs) is the HIGH byte of sat16(v >> (rs - 8)) (arithmetic shifts compose, and saturating to 16 bits commutes
		 * with dropping 8 more): two v_cvt_pk_i16_i32 and one v_perm_b32 per four values instead of four shift / clamp pairs.
		 * For rs < 8 the inner shift goes LEFT, which is exact only while v << (8 - rs) stays inside 32 bits: decided here from
		 * the layer's own weights and seeds. */
		if (M->mm && L->rs >= 0 && L->rs <= 31 && (L->rs >= 8 || (acc_bound[i] << (8 - L->rs)) < ((int64_t)1 << 31))) R->rs |= ED_RUN_RS_HI;
		R->in_n = L->in_n;
		R->in_off = pin; R->o_off = o_off;
		if (R->kind == ED_RUN_MERGE || R->kind == ED_RUN_CAT)
		{
			R->n_ks = SRC_N(i); R->koff_off = msrc0; R->ph = L->type; R->pitch_x = L->in_c;
			R->pix_per_img = st_h * st_w; R->col_w = st_w; R->out_c = L->out_c;
		}
		if (!held[st]) in_off = o_off; /* the consumer reads where this layer stored */
	}
	*frag = fb;
	*seeds = sb;
	mm->ok = 1;
	return EDISON_OK;
}
