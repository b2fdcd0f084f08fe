/*
 * mfcc_geom_frames.inc -- the body of the any-geometry MFCC kernels (mfcc_geom_kernels.hip): the frames of the call through stages 1-6,
 * for a kernel whose by-value argument is `ed_geom_args_t a`, whose template parameter is TEAM, and which defines
 * EDG_STORE(index, y) for what stage 6 does with the DCT row value y of element `index` of [n_frames][n_coef].
 *
 * Included textually, once per kernel, so that every kernel computes y by one source. A __forceinline__ function with the same body
 * changed the code of the existing int8 instances (the compiler simplifies a callee on its own before inlining it; one difference was
 * |X|^2 contracted to the other fma), and their instructions must stay as they were.
 */
	extern __shared__ __attribute__((aligned(16))) double edg_lds[];
	constexpr int TEAMS = EDG_BLOCK / TEAM;
	const int tid = TEAM == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
	const int team = TEAM == 64 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
	double *r0 = edg_lds + (size_t)team * (a.r0 + a.r1 + a.r2);
	double *r1 = r0 + a.r0, *mel = r1 + a.r1;
	const double2 *__restrict__ tw = reinterpret_cast<const double2 *>(a.tw);
	const int N = a.N, M = a.M, tws = a.packed ? 2 : 1;

	for (int g = blockIdx.x * TEAMS + team; g < a.n_frames; g += gridDim.x * TEAMS)
	{
		const int u = g / a.frames_per_utt, f = g - u * a.frames_per_utt;
		const int16_t *x = a.audio + (int64_t)u * a.utt_stride + (int64_t)f * a.frame_step;
		edg_sync<TEAM>(); /* the previous frame's DCT has read the mel bands */
		double *spec;
		if (M > 0)
		{
			/* ---- 1. load, 2. FFT */
			double2 *src = reinterpret_cast<double2 *>(r0), *dst = reinterpret_cast<double2 *>(r1);
			if (a.packed)
				for (int n = tid; n < M; n += TEAM) src[n] = make_double2((double)x[2 * n], (double)x[2 * n + 1]);
			else
				for (int n = tid; n < M; n += TEAM) src[n] = make_double2((double)x[n], 0.0);
			edg_sync<TEAM>();
			int ns = 1;
			for (int s = 0; s < a.n_stages; s++)
			{
				const int R = a.radix[s];
				if (R == 4) edg_stage<4, TEAM>(src, dst, M, ns, tws, tw, tid);
				else if (R == 2) edg_stage<2, TEAM>(src, dst, M, ns, tws, tw, tid);
				else if (R == 3) edg_stage<3, TEAM>(src, dst, M, ns, tws, tw, tid);
				else edg_stage<5, TEAM>(src, dst, M, ns, tws, tw, tid);
				edg_sync<TEAM>();
				double2 *t = src; src = dst; dst = t;
				ns *= R;
			}
			/* ---- 3. split, 4. spectrum: into the buffer the result is not in */
			spec = reinterpret_cast<double *>(dst);
			for (int k = tid; k < a.n_bins; k += TEAM)
			{
				double xr, xi;
				if (a.packed)
				{
					const double2 p = src[k < M ? k : k - M], q = src[k == 0 ? 0 : M - k]; /* Z[k mod M], Z[-k mod M] */
					const double er = 0.5 * (p.x + q.x), ei = 0.5 * (p.y - q.y);      /* E = (Z[k] + conj Z[-k]) / 2  */
					const double orr = 0.5 * (p.y + q.y), oi = -0.5 * (p.x - q.x);    /* O = (Z[k] - conj Z[-k]) / 2i */
					const double2 w = tw[k];
					xr = er + (orr * w.x - oi * w.y);
					xi = ei + (orr * w.y + oi * w.x);
				}
				else
				{
					xr = src[k].x;
					xi = src[k].y;
				}
				xr *= a.fft_scale;
				xi *= a.fft_scale;
				spec[k] = sqrt(xr * xr + xi * xi) * a.spec_scale;
			}
		}
		else
		{
			/* ---- 1. load, 2. direct DFT of the real frame: X[k] = sum_n x[n] W_N^(k n mod N), the index kept by addition */
			double *xs = r0;
			spec = r1;
			for (int n = tid; n < N; n += TEAM) xs[n] = (double)x[n];
			edg_sync<TEAM>();
			for (int k = tid; k < a.n_bins; k += TEAM)
			{
				double sr = 0.0, si = 0.0;
				int j = 0;
				for (int n = 0; n < N; n++)
				{
					const double v = xs[n];
					const double2 w = tw[j];
					sr = fma(v, w.x, sr);
					si = fma(v, w.y, si);
					j += k;
					if (j >= N) j -= N;
				}
				sr *= a.fft_scale;
				si *= a.fft_scale;
				spec[k] = sqrt(sr * sr + si * si) * a.spec_scale;
			}
		}
		edg_sync<TEAM>();

		/* ---- 5. mel bands over their nonzero taps, [ln] */
		for (int j = tid; j < a.n_mel; j += TEAM)
		{
			const int k0 = a.band[3 * j], len = a.band[3 * j + 1], off = a.band[3 * j + 2];
			double acc = 0.0;
			for (int t = 0; t < len; t++) acc = fma(spec[k0 + t], a.taps[off + t], acc);
			const double e = acc / a.mel_div;
			mel[j] = a.take_log ? log(e + 1e-6) : e;
		}
		edg_sync<TEAM>();

		/* ---- 6. DCT-II rows: y, stored by the including kernel's EDG_STORE */
		for (int c = tid; c < a.n_coef; c += TEAM)
		{
			const double *d = a.dct + (size_t)c * a.n_mel;
			double y = 0.0;
			for (int n = 0; n < a.n_mel; n++) y = fma(mel[n], d[n], y);
			y = y / a.dct_div;
			EDG_STORE((int64_t)g * a.n_coef + c, y);
		}
	}
