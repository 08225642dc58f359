// inverse.hip -- phase weighting, inverse frame CWT (real part), epilogue.
// Reference citations are relative to /root/reference/src.
#include "tspws_internal.h"
#include <hip/hip_ext.h>

// ------------------------------------------------------------------------------------------
// phase weighting (tspws_biased :909-943, tspws_unbiased :965-984)
// mode 0: wu==2 biased, 1: wu==1, 2: general power, 3: unbiased (K>1)
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_weight(double2 *__restrict__ OUT, const double2 *__restrict__ ST, const double2 *__restrict__ PS,
                                                size_t ncoef, int mode, double K, double M, double wu, const double *__restrict__ Mv,
                                                size_t y_out, size_t y_stack)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= ncoef) return;
	// blockIdx.y = independent stack (jackknife replica) with its own trace count M
	OUT += (size_t)blockIdx.y * y_out; ST += (size_t)blockIdx.y * y_stack; PS += (size_t)blockIdx.y * y_stack;
	if (Mv) M = Mv[blockIdx.y];
	OUT[i] = weight_value(ST[i], PS[i], mode, K, M, wu);
}

extern "C" int tspws_hip_weight(tspws_hip_plan *p, double *d_OUT, const double *d_ST, const double *d_PS, unsigned K, unsigned M,
                                double wu, int unbiased, void *s)
{
	if (!p || !d_OUT || !d_ST || !d_PS) return fail(TSPWS_E_ARG, "weight: NULL");
	HIP_TRY(hipSetDevice(p->device));
	const int mode = tspws_weight_mode(wu, unbiased, K);
	hipLaunchKernelGGL(k_weight, dim3((unsigned)((p->ncoef + 255) / 256)), dim3(256), 0, S_(s), (double2 *)d_OUT, (const double2 *)d_ST,
	                   (const double2 *)d_PS, p->ncoef, mode, (double)K, (double)M, wu, (const double *)nullptr, (size_t)0, (size_t)0);
	HIP_TRY(hipGetLastError());
	return 0;
}

int tspws_weight_mode(double wu, int unbiased, unsigned K)
{
	if (wu == 2 && unbiased && K != 1) return 3; // selection rule ts_pws1f_lib.c:226-228, K==1 falls back :972
	if (wu == 2) return 0;
	if (wu == 1) return 1;
	return 2;
}

void tspws_weight_batched(tspws_hip_plan *p, double2 *OUT, const double2 *ST, const double2 *PS, int mode, double K, double wu, const double *d_Mv,
                          unsigned nb, size_t y_out, size_t y_stack, hipStream_t st, double M)
{
	hipLaunchKernelGGL(k_weight, dim3((unsigned)((p->ncoef + 255) / 256), nb), dim3(256), 0, st, OUT, ST, PS, p->ncoef, mode, K, M, wu, d_Mv, y_out, y_stack);
}

// ------------------------------------------------------------------------------------------
// inverse frame transform, real part (gather form), generic:
//   x^[n] = sum_s gain_s * D_s * sum_{l: (n - cd + l) on the decimation grid} Re(conj(wd_s[l]) Y_s[.])
// with the grid restarting at the circular seam (cdotx.c:313-337); D==1 -> cdotx.c:176-211.
// One thread per output sample; NREC coefficient sets share the tap reads.
// ------------------------------------------------------------------------------------------
template <int NREC>
__global__ void __launch_bounds__(256) k_inverse_generic(const double2 *__restrict__ Y, size_t ncoef, unsigned N, const ScaleDesc *__restrict__ sc,
                                                         unsigned S, const double2 *__restrict__ wd, double *__restrict__ xout, int only_slow,
                                                         size_t y_coef, size_t y_out)
{
	const unsigned n = blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	Y += (size_t)blockIdx.y * y_coef; xout += (size_t)blockIdx.y * y_out; // blockIdx.y = independent reconstruction set
	double tot[NREC];
#pragma unroll
	for (int r = 0; r < NREC; r++) tot[r] = 0;
	for (unsigned s = 0; s < S; s++) {
		const ScaleDesc d = sc[s];
		if (only_slow && d.inv_fast) continue;
		const double2 *ws = wd + d.tap_off;
		const double2 *ys = Y + d.coef_off;
		long long n0 = (long long)n - d.cd;
		if (n0 < 0) n0 += N;
		const unsigned l0 = N - (unsigned)n0; // taps before the seam
		const unsigned lim = d.L < l0 ? d.L : l0;
		double acc[NREC];
#pragma unroll
		for (int r = 0; r < NREC; r++) acc[r] = 0;
		if (d.D > 1) {
			const unsigned D = d.D;
			unsigned l = (D - (unsigned)(n0 % D)) % D;
			unsigned q = (unsigned)((n0 + D - 1) / D);
			for (; l < lim; l += D, q++) {
				const double2 t = ws[l];
#pragma unroll
				for (int r = 0; r < NREC; r++) {
					const double2 y = ys[(size_t)r * ncoef + q];
					acc[r] = fma(t.x, y.x, fma(t.y, y.y, acc[r]));
				}
			}
			q = 0;
			for (l = l0; l < d.L; l += D, q++) {
				const double2 t = ws[l];
#pragma unroll
				for (int r = 0; r < NREC; r++) {
					const double2 y = ys[(size_t)r * ncoef + q];
					acc[r] = fma(t.x, y.x, fma(t.y, y.y, acc[r]));
				}
			}
#pragma unroll
			for (int r = 0; r < NREC; r++) tot[r] += d.gain * ((double)D * acc[r]);
		} else {
			for (unsigned l = 0; l < lim; l++) {
				const double2 t = ws[l];
#pragma unroll
				for (int r = 0; r < NREC; r++) {
					const double2 y = ys[(size_t)r * ncoef + (unsigned)n0 + l];
					acc[r] = fma(t.x, y.x, fma(t.y, y.y, acc[r]));
				}
			}
			for (unsigned l = lim; l < d.L; l++) {
				const double2 t = ws[l];
#pragma unroll
				for (int r = 0; r < NREC; r++) {
					const double2 y = ys[(size_t)r * ncoef + (l - l0)];
					acc[r] = fma(t.x, y.x, fma(t.y, y.y, acc[r]));
				}
			}
#pragma unroll
			for (int r = 0; r < NREC; r++) tot[r] += d.gain * acc[r];
		}
	}
#pragma unroll
	for (int r = 0; r < NREC; r++) xout[(size_t)r * N + n] = tot[r];
}

#include "inv_poly.h"
#include "batch_host.h"

// octaves up to this decimation take the LDS-staged instantiation (TSPWS_INV_LDS_MAXD, default 1: the full-rate scales of the
// Mexican hat / `uni` frames, whose per-lane windows touch 64 cache lines per wave-load; 0: none)
static unsigned inv_lds_maxd()
{
	static int v = -1;
	if (v < 0) { const char *e = sweep_env("TSPWS_INV_LDS_MAXD"); v = e ? std::max(0, atoi(e)) : 1; }
	return (unsigned)v;
}

// work list of the polyphase inverse: one item group per run of consecutive scales with the same D (an octave: its voices are
// summed in registers).  SHORT frames -- all octave items together fewer than 768 waves, i.e. N < ~28 000 for the default frames --
// get one item per SCALE instead: the kernel is a chain of dependent round trips per voice, and with less than two waves per SIMD
// nothing hides them (N = 16501: 105 workgroups on 256 CUs); four times the waves, each a quarter as long, and the combining
// kernel adds a row per scale (TSPWS_INV_SPLIT=0 / 1 forces either form).  Long frames fill the chip with octave items (round 1:
// the voices on separate waves 49 vs 50 us at N = 131072).
int tspws_build_inverse(tspws_hip_plan *p)
{
	std::vector<OctDesc> oc;
	unsigned woff = 0;
	p->inv_ngeneric = 0;
	p->og_s0.clear(); p->og_nv.clear();
	bool split = false;
	{
		unsigned waves = 0;
		for (unsigned s = 0; s < p->S;) {
			unsigned e = s + 1;
			while (e < p->S && p->sc[e].D == p->sc[s].D) e++;
			p->og_s0.push_back(s); p->og_nv.push_back(e - s); // the octaves themselves: what a share of the sharded finish is made of
			const unsigned D = p->sc[s].D, dl = D >= 64 ? 64u : std::max(1u, 1u << (unsigned)ceil(log2((double)std::max(1u, D))));
			const unsigned NG = (p->sc[s].Ns + INV_R - 1) / INV_R, GW = 64 / dl;
			waves += (D > 64 ? (D + 63) / 64 : 1) * ((NG + GW - 1) / GW);
			s = e;
		}
		split = waves < 768; // (tools/experiments/inv_split.sh: 499 x 16501 two-stage 0.157 -> 0.134 ms, 64 x 8192 0.165 -> 0.158; N = 32768 / 65536 / 131072 unchanged or worse)
		if (const char *e = sweep_env("TSPWS_INV_SPLIT")) split = atoi(e) != 0;
	}
	for (unsigned s = 0; s < p->S;) {
		unsigned e = s + 1;
		while (!split && e < p->S && p->sc[e].D == p->sc[s].D) e++;
		OctDesc o;
		memset(&o, 0, sizeof o);
		o.gen = p->sc[s].inv_fast ? 0u : 1u;
		o.s0 = s; o.nv = e - s; o.D = p->sc[s].D; o.Ns = p->sc[s].Ns;
		unsigned dl = 1, lg = 0;
		while (dl < o.D && dl < 64) { dl <<= 1; lg++; }
		o.DL = dl; o.logDL = lg;
		o.MC = o.D > 64 ? (o.D + 63) / 64 : 1;
		const unsigned NG = (o.Ns + INV_R - 1) / INV_R, GW = 64 / o.DL;
		o.ngw = (NG + GW - 1) / GW;
		oc.push_back(o);
		s = e;
	}
	// octaves whose decimation divides N first: the two classes are launched separately (k_inv_poly<., GEN>)
	std::stable_sort(oc.begin(), oc.end(), [](const OctDesc &x, const OctDesc &y) { return x.gen < y.gen; });
	p->inv_waves_fast = 0; p->inv_waves_lds = 0;
	for (size_t i = 0; i < oc.size(); i++) {
		oc[i].wave_off = woff; oc[i].slot = (unsigned)i;
		woff += oc[i].MC * oc[i].ngw;
		if (!oc[i].gen) p->inv_waves_fast = woff;
		// the finely decimated octaves (D < 64) come first in scale order: their waves take the LDS-staged instantiation
		if (!oc[i].gen && oc[i].D <= inv_lds_maxd() && p->inv_waves_lds == oc[i].wave_off) p->inv_waves_lds = woff;
	}
	if (const char *e = sweep_env("TSPWS_INV_LDS")) if (*e == '0') p->inv_waves_lds = 0; // (A/B: the per-lane form for every octave)
	p->inv_waves = woff; p->inv_noct = (unsigned)oc.size();
	p->oc_s0.clear(); p->oc_nv.clear(); p->oc_wave_off.clear(); p->oc_nwaves.clear(); p->oc_gen.clear();
	for (const OctDesc &o : oc) {
		p->oc_s0.push_back(o.s0); p->oc_nv.push_back(o.nv); p->oc_wave_off.push_back(o.wave_off); p->oc_nwaves.push_back(o.MC * o.ngw);
		p->oc_gen.push_back(o.gen);
	}
	if (!oc.empty()) {
		HIP_TRY(hipMalloc(&p->d_oc, oc.size() * sizeof(OctDesc)));
		HIP_TRY(hipMemcpy(p->d_oc, oc.data(), oc.size() * sizeof(OctDesc), hipMemcpyHostToDevice));
	}
	return 0;
}

#if FL_ABLATE
// debug build only: only the octave classes of k_inv_poly named by the hex mask TSPWS_INV_CLASSES run (results wrong: timing ablation)
extern "C" int tspws_hip_inv_ablate(void)
{
	if (const char *e = sweep_env("TSPWS_INV_CLASSES")) {
		const unsigned m = (unsigned)strtoul(e, nullptr, 16);
		HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(inv_class_mask), &m, sizeof m));
	}
	return 0;
}
#endif

bool tspws_generic_inverse()
{
	static int v = -1;
	if (v < 0) { const char *e = sweep_env("TSPWS_INV_GENERIC"); v = (e && *e == '1') ? 1 : 0; }
	return v == 1;
}

// The waves [w0, w1) of the polyphase inverse's launch list for nb NREC-set reconstructions (grid.y) on `st`, into the octave buffer (*obuf: inv_nslots
// rows per set): the LDS-staged instantiation below the LDS bound, the per-lane one up to inv_waves_fast, the GEN one above.
static unsigned inv_nslots(const tspws_hip_plan *p) { return p->inv_noct + (p->inv_ngeneric ? 1 : 0); }
// Bytes that one row (coefficient set) of a batched tspws_hip_inverse costs in its largest block: the set itself, its reconstruction, or its
// share of the octave buffer below (N doubles per octave item, + 1 for the generic scales whether or not the frame has any: an upper bound).
// What the batched units size their finish batches by.
size_t tspws_inverse_row_bytes(const tspws_hip_plan *p)
{
	return std::max({p->ncoef * sizeof(double2), (size_t)p->N * sizeof(double), (size_t)(p->inv_noct + 1) * p->N * sizeof(double)});
}
template <int NREC>
static int inv_launch_waves(tspws_hip_plan *p, const double2 *Y, unsigned nb, unsigned w0, unsigned w1, hipStream_t st, double **obuf)
{
	const size_t slot = (size_t)NREC * p->N, y_coef = (size_t)NREC * p->ncoef, y_obuf = (size_t)inv_nslots(p) * slot;
	void *v;
	if (int rc = scratch(p, SCR_OBUF, (size_t)nb * y_obuf * sizeof(double), &v)) return rc;
	double *ob = *obuf = (double *)v;
	// the LDS-staged octaves (D = 1: two 80-KB workgroups per CU) run BESIDE the others (latency-bound, eight waves per SIMD) on the
	// plan's side stream: one after the other they took 64 + 153 us for cfg4's twelve reconstructions, the single per-lane launch 262
	// (batched reconstructions only: a single pair is 206 vs 197 us that way -- the fork / join and two waves per SIMD cost more than
	// the one octave's coalescing gains)
	const unsigned lds_w = nb >= 2 ? p->inv_waves_lds : 0u;
	const unsigned wl = std::min(std::max(lds_w, w0), w1), wf = std::min(std::max(p->inv_waves_fast, wl), w1); // LDS-staged [w0, wl), per-lane [wl, wf), GEN [wf, w1)
	const bool beside = wl > w0 && wf > wl;
	if (beside) if (int rc = tspws_fork(p, st, p->side, p->ev_fork)) return rc;
	if (wl > w0)
		hipLaunchKernelGGL((k_inv_poly<NREC, false, true>), dim3((wl - w0 + 3) / 4, nb), dim3(256), 0, beside ? p->side : st, Y, p->ncoef, p->N, p->d_sc, p->d_oc,
		                   p->inv_noct, p->d_wd, ob, slot, wl, y_coef, y_obuf, w0);
	if (wf > wl)
		hipLaunchKernelGGL((k_inv_poly<NREC, false>), dim3((wf - wl + 3) / 4, nb), dim3(256), 0, st, Y, p->ncoef, p->N, p->d_sc, p->d_oc, p->inv_noct, p->d_wd, ob,
		                   slot, wf, y_coef, y_obuf, wl);
	if (w1 > wf)
		hipLaunchKernelGGL((k_inv_poly<NREC, true>), dim3((w1 - wf + 3) / 4, nb), dim3(256), 0, st, Y, p->ncoef, p->N, p->d_sc, p->d_oc, p->inv_noct, p->d_wd, ob,
		                   slot, w1, y_coef, y_obuf, wf);
	if (beside) return tspws_join(p->side, st, p->ev_join);
	return 0;
}

// nb independent NREC-set reconstructions in one launch (grid.y): set j reads Y + j NREC ncoef, writes x + j NREC N
// f_ts / f_ls (NREC == 2, nb == 1 only): the stack's float outputs are written by the combining kernel itself (no FP64
// reconstructions in memory, no epilogue launch); x may then be NULL.
template <int NREC>
static int inverse_launch(tspws_hip_plan *p, const double2 *Y, double *x, hipStream_t st, unsigned nb = 1, float *f_ts = nullptr, float *f_ls = nullptr,
                          float f_mtr = 1.0f)
{
	const unsigned nbx = (p->N + 255) / 256;
	const size_t slot = (size_t)NREC * p->N;
	if (tspws_generic_inverse() || p->inv_noct == 0) {
		hipLaunchKernelGGL(k_inverse_generic<NREC>, dim3(nbx, nb), dim3(256), 0, st, Y, p->ncoef, p->N, p->d_sc, p->S, p->d_wd, x, 0,
		                   (size_t)NREC * p->ncoef, slot);
		return 0;
	}
	const unsigned nslots = inv_nslots(p);
	double *obuf;
	if (int rc = inv_launch_waves<NREC>(p, Y, nb, 0, p->inv_waves, st, &obuf)) return rc;
	if (p->inv_ngeneric)
		hipLaunchKernelGGL(k_inverse_generic<NREC>, dim3(nbx, nb), dim3(256), 0, st, Y, p->ncoef, p->N, p->d_sc, p->S, p->d_wd,
		                   obuf + (size_t)p->inv_noct * slot, 1, (size_t)NREC * p->ncoef, (size_t)nslots * slot);
	if (NREC == 2 && nb == 1 && (f_ts || f_ls))
		if (hipEvent_t e1 = p->le.call_end) { // the call's end event rides on its last launch (tspws_hip_stack)
			p->le.call_end = nullptr;
			hipExtLaunchKernelGGL(k_inv_combine_out, dim3(nbx, 2), dim3(256), 0, st, nullptr, e1, 0, (const double *)obuf, slot, nslots, (size_t)p->N, f_ts, f_ls, f_mtr);
		} else
			hipLaunchKernelGGL(k_inv_combine_out, dim3(nbx, 2), dim3(256), 0, st, obuf, slot, nslots, (size_t)p->N, f_ts, f_ls, f_mtr);
	else
		hipLaunchKernelGGL(k_inv_combine, dim3((unsigned)((slot + 255) / 256), nb), dim3(256), 0, st, obuf, slot, nslots, slot, x,
		                   (size_t)nslots * slot, slot);
	return 0;
}

extern "C" int tspws_hip_inverse(tspws_hip_plan *p, const double *d_Y, size_t nrec, double *d_x, void *s)
{
	if (!p || !d_Y || !d_x) return fail(TSPWS_E_ARG, "inverse: NULL");
	HIP_TRY(hipSetDevice(p->device));
	int rc;
	const size_t pairs = nrec / 2;
	for (size_t r = 0; r < pairs; r += 32768) { // pairs of coefficient sets share the tap reads; all pairs in one launch
		const unsigned nb = (unsigned)std::min<size_t>(pairs - r, 32768);
		if ((rc = inverse_launch<2>(p, (const double2 *)d_Y + 2 * r * p->ncoef, d_x + 2 * r * p->N, S_(s), nb))) return rc;
	}
	if (nrec & 1)
		if ((rc = inverse_launch<1>(p, (const double2 *)d_Y + (nrec - 1) * p->ncoef, d_x + (nrec - 1) * p->N, S_(s)))) return rc;
	HIP_TRY(hipGetLastError());
	return 0;
}

extern "C" int tspws_hip_inverse_info(const tspws_hip_plan *p, tspws_hip_inverse_info_t *info)
{
	if (!p || !info) return fail(TSPWS_E_ARG, "inverse_info: NULL");
	info->items = p->inv_noct;
	info->per_scale = p->inv_noct == p->S ? 1u : 0u;
	info->waves = p->inv_waves; info->waves_lds = p->inv_waves_lds; info->waves_fast = p->inv_waves_fast;
	info->generic = (tspws_generic_inverse() || p->inv_noct == 0) ? 1u : 0u;
	return 0;
}

// ------------------------------------------------------------------------------------------
// band rows (include/tspws_hip.h: tspws_hip_inverse_bands; kernels: inv_poly.h)
// ------------------------------------------------------------------------------------------
// The per-scale work list -- one item per scale, the geometry of the `split` form of tspws_build_inverse whatever the frame's length -- is built
// at the first band call and kept here, apart from d_oc: the list tspws_hip_inverse launches is not touched.  A call selects the scales inside at
// least one band (scale order inside a class, D divides N first: the launch classes of inv_launch_waves), gives them consecutive waves and the
// slot rows 0 .. U - 1 in scale order, and uploads that list and the bands' slot ranges; the device copies are the plan's, so a call with another
// table than the last one waits for the stream first, and a call with the same table uploads nothing.
struct BandTables {
	std::vector<OctDesc> per_scale;  // item of every scale (wave_off / slot are set per table)
	std::vector<tspws_band> table;   // the table the device copies were made for
	bool valid = false;
	unsigned U = 0, waves = 0, waves_lds = 0, waves_fast = 0;
	OctDesc *d_oc = nullptr;         // [S]
	BandSlots *d_bt = nullptr;       // [TSPWS_MAX_BANDS]
};

void tspws_bands_destroy(tspws_hip_plan *p)
{
	if (!p->bands) return;
	if (p->bands->d_oc) (void)hipFree(p->bands->d_oc);
	if (p->bands->d_bt) (void)hipFree(p->bands->d_bt);
	delete p->bands;
	p->bands = nullptr;
}

// what a band table is refused for; the checks that need no plan come first (p / bands NULL: what needs them is left out -- the entry points
// refuse the NULL itself afterwards)
int tspws_bands_check(const tspws_hip_plan *p, const tspws_band *bands, unsigned R, const char *who)
{
	const std::string w(who);
	if (R > TSPWS_MAX_BANDS) return fail(TSPWS_E_ARG, (w + ": more than 1024 bands").c_str());
	if (!bands) return 0;
	for (unsigned r = 0; r < R; r++)
		if (bands[r].s_begin > bands[r].s_end) return fail(TSPWS_E_ARG, (w + ": a band with s_begin > s_end").c_str());
	if (!p) return 0;
	for (unsigned r = 0; r < R; r++)
		if (bands[r].s_end > p->S) return fail(TSPWS_E_ARG, (w + ": a band ends behind the last scale").c_str());
	return 0;
}

static int bands_setup(tspws_hip_plan *p, const tspws_band *bands, unsigned R, hipStream_t st)
{
	if (!p->bands) {
		BandTables *t = new BandTables;
		p->bands = t;
		for (unsigned s = 0; s < p->S; s++) {
			OctDesc o;
			memset(&o, 0, sizeof o);
			o.gen = p->sc[s].inv_fast ? 0u : 1u;
			o.s0 = s; o.nv = 1; o.D = p->sc[s].D; o.Ns = p->sc[s].Ns;
			unsigned dl = 1, lg = 0;
			while (dl < o.D && dl < 64) { dl <<= 1; lg++; }
			o.DL = dl; o.logDL = lg;
			o.MC = o.D > 64 ? (o.D + 63) / 64 : 1;
			const unsigned NG = (o.Ns + INV_R - 1) / INV_R, GW = 64 / o.DL;
			o.ngw = (NG + GW - 1) / GW;
			t->per_scale.push_back(o);
		}
		HIP_TRY(hipMalloc(&t->d_oc, std::max<size_t>(1, p->S) * sizeof(OctDesc)));
		HIP_TRY(hipMalloc(&t->d_bt, TSPWS_MAX_BANDS * sizeof(BandSlots)));
	}
	BandTables &t = *p->bands;
	if (t.valid && t.table.size() == R && (!R || !memcmp(t.table.data(), bands, R * sizeof(tspws_band)))) return 0;
	t.valid = false;
	std::vector<unsigned> rank(p->S + 1, 0); // scales with work items below s
	{
		std::vector<char> in(p->S, 0);
		for (unsigned r = 0; r < R; r++)
			for (unsigned s = bands[r].s_begin; s < bands[r].s_end; s++) in[s] = 1;
		for (unsigned s = 0; s < p->S; s++) rank[s + 1] = rank[s] + (in[s] ? 1u : 0u);
	}
	std::vector<OctDesc> oc;
	for (unsigned s = 0; s < p->S; s++)
		if (rank[s + 1] > rank[s]) { oc.push_back(t.per_scale[s]); oc.back().slot = rank[s]; }
	std::stable_sort(oc.begin(), oc.end(), [](const OctDesc &x, const OctDesc &y) { return x.gen < y.gen; });
	unsigned woff = 0;
	t.waves_fast = t.waves_lds = 0;
	for (OctDesc &o : oc) {
		o.wave_off = woff;
		woff += o.MC * o.ngw;
		if (!o.gen) t.waves_fast = woff;
		if (!o.gen && o.D <= inv_lds_maxd() && t.waves_lds == o.wave_off) t.waves_lds = woff; // (the finely decimated scales come first, as in tspws_build_inverse)
	}
	if (const char *e = sweep_env("TSPWS_INV_LDS")) if (*e == '0') t.waves_lds = 0;
	t.waves = woff; t.U = (unsigned)oc.size();
	std::vector<BandSlots> bt(R);
	for (unsigned r = 0; r < R; r++) { bt[r].slot0 = rank[bands[r].s_begin]; bt[r].n = bands[r].s_end - bands[r].s_begin; } // (every scale of a band has a row)
	HIP_TRY(hipStreamSynchronize(st)); // an earlier call on this stream may still read the tables
	if (!oc.empty()) HIP_TRY(hipMemcpy(t.d_oc, oc.data(), oc.size() * sizeof(OctDesc), hipMemcpyHostToDevice));
	if (R) HIP_TRY(hipMemcpy(t.d_bt, bt.data(), R * sizeof(BandSlots), hipMemcpyHostToDevice));
	t.table.assign(bands, bands + R);
	t.valid = true;
	return 0;
}

// the waves of the band table's list for nb groups of NREC sets (grid.y), as inv_launch_waves: the LDS-staged scales beside the others when there are both
template <int NREC, bool QUAD>
static int bands_launch_waves(tspws_hip_plan *p, const double2 *Y, unsigned nb, double *ob, size_t y_obuf, size_t q_off, hipStream_t st)
{
	const BandTables &t = *p->bands;
	const size_t slot = (size_t)NREC * p->N, y_coef = (size_t)NREC * p->ncoef;
	const unsigned wl = nb >= 2 ? t.waves_lds : 0u, wf = t.waves_fast, w1 = t.waves;
	const bool beside = wl > 0 && wf > wl;
	if (beside) if (int rc = tspws_fork(p, st, p->side, p->ev_fork)) return rc;
	if (wl > 0)
		hipLaunchKernelGGL((k_inv_poly<NREC, false, true, QUAD>), dim3((wl + 3) / 4, nb), dim3(256), 0, beside ? p->side : st, Y, p->ncoef, p->N, p->d_sc,
		                   (const OctDesc *)t.d_oc, t.U, p->d_wd, ob, slot, wl, y_coef, y_obuf, 0u, q_off);
	if (wf > wl)
		hipLaunchKernelGGL((k_inv_poly<NREC, false, false, QUAD>), dim3((wf - wl + 3) / 4, nb), dim3(256), 0, st, Y, p->ncoef, p->N, p->d_sc, (const OctDesc *)t.d_oc,
		                   t.U, p->d_wd, ob, slot, wf, y_coef, y_obuf, wl, q_off);
	if (w1 > wf)
		hipLaunchKernelGGL((k_inv_poly<NREC, true, false, QUAD>), dim3((w1 - wf + 3) / 4, nb), dim3(256), 0, st, Y, p->ncoef, p->N, p->d_sc, (const OctDesc *)t.d_oc,
		                   t.U, p->d_wd, ob, slot, w1, y_coef, y_obuf, wf, q_off);
	if (beside) return tspws_join(p->side, st, p->ev_join);
	return 0;
}

int tspws_inverse_bands_run(tspws_hip_plan *p, const double2 *Y, size_t nset, const tspws_band *bands, unsigned R, const BandOut &out, hipStream_t st,
                            unsigned *finish_batches, unsigned *scales)
{
	if (int rc = bands_setup(p, bands, R, st)) return rc;
	const BandTables &t = *p->bands;
	const bool f32 = out.ts != nullptr, quad = f32 ? out.ts_env != nullptr : out.im != nullptr;
	const size_t N = p->N, UN = (size_t)t.U * N;
	if (scales) *scales = t.U;
	// sets per finish batch: their slot rows (U x N doubles per set, twice that with the quadrature) within the parts budget; even, so that
	// the pairs are the same whatever the batching
	const size_t per_set = std::max<size_t>(1, (quad ? 2 : 1) * UN) * sizeof(double);
	const size_t batch = even_rows_per_batch(tspws_part_budget_bytes(), per_set, std::max<size_t>(nset, 2));
	const unsigned nbx = (unsigned)((N + 255) / 256);
	for (size_t j0 = 0; j0 < nset; j0 += batch) {
		const unsigned ns = (unsigned)std::min(batch, nset - j0), pairs = quad ? 0u : ns / 2;
		if (finish_batches) ++*finish_batches;
		void *v;
		if (int rc = scratch(p, SCR_OBUF, (size_t)ns * per_set, &v)) return rc;
		double *ob = (double *)v;
		const double2 *Yb = Y + j0 * p->ncoef;
		if (t.waves) {
			int rc = 0;
			if (quad) rc = bands_launch_waves<1, true>(p, Yb, ns, ob, 2 * UN, UN, st);
			else {
				if (pairs) rc = bands_launch_waves<2, false>(p, Yb, pairs, ob, 2 * UN, 0, st);
				if (!rc && (ns & 1)) rc = bands_launch_waves<1, false>(p, Yb + (size_t)(ns - 1) * p->ncoef, 1, ob + (size_t)pairs * 2 * UN, UN, 0, st);
			}
			if (rc) return rc;
		}
		BandCombine a;
		a.N = N; a.U = t.U; a.paired = 2 * pairs; a.set0 = (unsigned)j0; a.quad = quad ? 1u : 0u;
		a.bt = t.d_bt;
		a.re = out.re; a.im = out.im;
		a.ts = out.ts; a.ls = out.ls; a.ts_env = out.ts_env; a.ls_env = out.ls_env;
		a.row = out.d_row; a.cnt = out.d_cnt; a.row0 = out.row0; a.cnt0 = out.cnt0;
		if (f32) hipLaunchKernelGGL(k_inv_combine_bands<true>, dim3(nbx, R, ns), dim3(256), 0, st, (const double *)ob, a);
		else hipLaunchKernelGGL(k_inv_combine_bands<false>, dim3(nbx, R, ns), dim3(256), 0, st, (const double *)ob, a);
	}
	HIP_TRY(hipGetLastError());
	return 0;
}

extern "C" int tspws_hip_inverse_bands(tspws_hip_plan *p, const double *d_Y, size_t nset, const tspws_band *h_bands, unsigned R, double *d_re, double *d_im,
                                       void *s)
{
	if (int rc = tspws_bands_check(p, h_bands, R, "inverse_bands")) return rc;
	if (!p) return fail(TSPWS_E_ARG, "inverse_bands: NULL");
	if (!R || !nset) return 0;
	if (!d_Y || !h_bands || !d_re) return fail(TSPWS_E_ARG, "inverse_bands: NULL");
	HIP_TRY(hipSetDevice(p->device));
	BandOut out;
	out.re = d_re; out.im = d_im;
	return tspws_inverse_bands_run(p, (const double2 *)d_Y, nset, h_bands, R, out, S_(s), nullptr, nullptr);
}

extern "C" int tspws_bands_from_frequencies(const double *scale, unsigned S, double w0, double dt, const double *f_lo, const double *f_hi, unsigned R,
                                            tspws_band *bands, double *fc)
{
	if (!scale && S) return fail(TSPWS_E_ARG, "bands_from_frequencies: NULL");
	if (R && (!f_lo || !f_hi || !bands)) return fail(TSPWS_E_ARG, "bands_from_frequencies: NULL");
	if (!(dt > 0) || !std::isfinite(dt)) return fail(TSPWS_E_ARG, "bands_from_frequencies: dt must be positive");
	for (unsigned r = 0; r < R; r++) {
		if (!std::isfinite(f_lo[r]) || !std::isfinite(f_hi[r])) return fail(TSPWS_E_ARG, "bands_from_frequencies: a band edge is not finite");
		if (f_lo[r] > f_hi[r]) return fail(TSPWS_E_ARG, "bands_from_frequencies: f_lo > f_hi");
	}
	auto centre = [&](unsigned s) { return w0 / (2 * TSPWS_PI * dt * scale[s]); }; // ts_pws1f_lib.c:112
	if (fc) for (unsigned s = 0; s < S; s++) fc[s] = centre(s);
	for (unsigned r = 0; r < R; r++) {
		// fc decreases with s: [first s with fc_s < f_hi, first s with fc_s < f_lo)
		unsigned a = 0, b;
		while (a < S && !(centre(a) < f_hi[r])) a++;
		b = a;
		while (b < S && !(centre(b) < f_lo[r])) b++;
		bands[r].s_begin = a; bands[r].s_end = b;
	}
	return 0;
}

// Batched pairs of reconstructions in TWO halves (the one-pass stack + jackknife call, resample.hip): the octaves of the scales [0, s_split) --
// those the FIR forward kernels completed -- EARLY, on the stream `early` on which their weighted coefficient sets are complete, beside whatever
// the caller's stream still runs (the spectral chain of the other scales: its tail is a run of short, latency-bound kernels); the other octaves
// and the combining kernel LATE, on the caller's stream once it has been made to wait for `early`.  The octave items are independent (one row
// of the octave buffer each), so the halves are two wave ranges of the same launch list.  *done = false: this plan / call has no such split
// (generic octaves, a single reconstruction, octave items not in scale order) -- the caller takes tspws_hip_inverse.
static bool inv_split_point(const tspws_hip_plan *p, unsigned s_split, unsigned *w_split)
{
	if (tspws_generic_inverse() || !p->inv_noct || p->inv_ngeneric || p->inv_waves_fast != p->inv_waves) return false;
	unsigned w = p->inv_waves_fast;
	for (unsigned i = 0; i < p->inv_noct; i++) {
		if (i && p->oc_s0[i] < p->oc_s0[i - 1]) return false;
		if (p->oc_s0[i] < s_split && p->oc_s0[i] + p->oc_nv[i] > s_split) return false; // (an octave item across the split)
		if (p->oc_s0[i] >= s_split) { w = p->oc_wave_off[i]; break; }
	}
	*w_split = w;
	return w > 0 && w < p->inv_waves_fast && p->inv_waves_lds <= w;
}

int tspws_inverse_pairs_early(tspws_hip_plan *p, const double2 *Y, unsigned nb, unsigned s_split, hipStream_t early, bool *done)
{
	*done = false;
	unsigned w_split = 0;
	double *obuf;
	if (nb < 2 || !inv_split_point(p, s_split, &w_split)) return 0;
	if (int rc = inv_launch_waves<2>(p, Y, nb, 0, w_split, early, &obuf)) return rc; // (the LDS-staged octaves beside the per-lane ones, as in inverse_launch)
	HIP_TRY(hipGetLastError());
	*done = true;
	return 0;
}

int tspws_inverse_pairs_late(tspws_hip_plan *p, const double2 *Y, double *x, unsigned nb, unsigned s_split, hipStream_t st)
{
	unsigned w_split = 0;
	if (nb < 2 || !inv_split_point(p, s_split, &w_split)) return fail(TSPWS_E_ARG, "inverse_pairs_late: no early half was launched");
	const size_t slot = (size_t)2 * p->N;
	double *obuf;
	if (int rc = inv_launch_waves<2>(p, Y, nb, w_split, p->inv_waves_fast, st, &obuf)) return rc;
	hipLaunchKernelGGL(k_inv_combine, dim3((unsigned)((slot + 255) / 256), nb), dim3(256), 0, st, obuf, slot, p->inv_noct, slot, x, (size_t)p->inv_noct * slot, slot);
	HIP_TRY(hipGetLastError());
	return 0;
}

// Two reconstructions (sets 0 and 1 of Y) from the scales [s_lo, s_hi) ONLY -- whole decimation octaves -- as FP64 partial
// sums x2[2][N]: the reconstruction is a sum over scales, so the shares of disjoint scale ranges add up to the whole.
int tspws_inverse_scales(tspws_hip_plan *p, const double2 *Y, double *x2, hipStream_t st, ScaleRange rg)
{
	const unsigned s_lo = rg.s0, s_hi = rg.s1;
	const size_t slot = 2 * (size_t)p->N;
	double *obuf = nullptr;
	// the octave items are stored class by class (decimation divides N first), in scale order inside a class: the items
	// of a scale range are one contiguous run per class
	unsigned first[2] = {~0u, ~0u}, last[2] = {0, 0};
	for (unsigned i = 0; i < p->inv_noct; i++) {
		if (p->oc_s0[i] < s_lo || p->oc_s0[i] >= s_hi) continue;
		const unsigned c = p->oc_gen[i] ? 1u : 0u;
		if (first[c] == ~0u) first[c] = i;
		last[c] = i;
	}
	for (unsigned c = 0; c < 2; c++) {
		if (first[c] == ~0u) continue;
		if (int rc = inv_launch_waves<2>(p, Y, 1, p->oc_wave_off[first[c]], p->oc_wave_off[last[c]] + p->oc_nwaves[last[c]], st, &obuf)) return rc;
	}
	const unsigned a0 = first[0] == ~0u ? 0u : first[0], na = first[0] == ~0u ? 0u : last[0] - first[0] + 1;
	const unsigned b0 = first[1] == ~0u ? 0u : first[1], nb = first[1] == ~0u ? 0u : last[1] - first[1] + 1;
	hipLaunchKernelGGL(k_inv_combine_ranges, dim3((unsigned)((slot + 255) / 256)), dim3(256), 0, st, (const double *)obuf, slot, a0, na, b0, nb, slot, x2);
	HIP_TRY(hipGetLastError());
	return 0;
}

// epilogue, ts_pws1f_lib.c:233-241 (ls is a FLOAT division by the converted trace count)
__global__ void __launch_bounds__(256) k_epilogue(float *__restrict__ ls, float *__restrict__ ts, const double *__restrict__ xst,
                                                  const double *__restrict__ xout, size_t N, float mtr)
{
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const size_t o = (size_t)blockIdx.y * N; // blockIdx.y = row of a batch of outputs
	if (ls) ls[o + n] = (float)xst[o + n] / mtr;
	if (ts) ts[o + n] = (float)xout[o + n];
}

extern "C" int tspws_hip_epilogue(float *d_ls, float *d_ts, const double *d_xst, const double *d_xout, size_t N, unsigned mtr, void *s)
{
	if ((d_ls && !d_xst) || (d_ts && !d_xout)) return fail(TSPWS_E_ARG, "epilogue: NULL");
	hipLaunchKernelGGL(k_epilogue, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, S_(s), d_ls, d_ts, d_xst, d_xout, N, (float)mtr);
	HIP_TRY(hipGetLastError());
	return 0;
}

void tspws_epilogue_rows(float *d_ts, const double *d_x, size_t N, unsigned nb, hipStream_t st)
{
	hipLaunchKernelGGL(k_epilogue, dim3((unsigned)((N + 255) / 256), nb), dim3(256), 0, st, (float *)nullptr, d_ts, (const double *)nullptr, d_x, N, 1.0f);
}

// The stack's two reconstructions: set 0 = ICWT(OUT) -> tsPWS, set 1 = ICWT(ST) -> ls (float division by the trace count); the
// combining kernel of the polyphase inverse writes the floats itself.
int tspws_inverse_pair_out(tspws_hip_plan *p, const double2 *Y, float *d_ts, float *d_ls, float mtr, hipStream_t st)
{
	int rc;
	if (!tspws_generic_inverse() && p->inv_noct) {
		if ((rc = inverse_launch<2>(p, Y, nullptr, st, 1, d_ts, d_ls, mtr))) return rc;
		HIP_TRY(hipGetLastError());
		return 0;
	}
	void *v;
	if ((rc = scratch(p, SCR_X2, 2 * (size_t)p->N * sizeof(double), &v))) return rc;
	double *x2 = (double *)v;
	if ((rc = tspws_hip_inverse(p, (const double *)Y, 2, x2, (void *)st))) return rc; // row 0 = ICWT(OUT), row 1 = ICWT(ST)
	hipLaunchKernelGGL(k_epilogue, dim3((unsigned)((p->N + 255) / 256)), dim3(256), 0, st, d_ls, d_ts, (const double *)(x2 + p->N), (const double *)x2, (size_t)p->N, mtr);
	HIP_TRY(hipGetLastError());
	return 0;
}
