// hd_selftest.hip -- device self-test of the wave primitives every kernel leans
// on (DPP prefix scan, strided CRC folding, slot arithmetic).  Run by
// hipdeflate_selftest(); tests/test_gpu_selftest.py calls it on the GPU box.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/hipdeflate.h"
#include "hd_device.hpp"
#include "hd_deflate_dynamic.hpp"

namespace {

__global__ __launch_bounds__(64) void k_selftest_scan(const uint32_t *x, uint32_t *incl)
{
	incl[blockIdx.x * 64 + threadIdx.x] = hd::wave_incl_scan(x[blockIdx.x * 64 + threadIdx.x]);
}

__global__ __launch_bounds__(64) void k_selftest_slots(uint32_t *out)
{
	// out[len]   = packed (sym, eb, ev) for len 3..258; out[512 + i] for a sweep of offsets
	for (uint32_t len = 3 + threadIdx.x; len <= 258; len += 64) {
		uint32_t s, eb, ev;
		hd::len_slot(len, s, eb, ev);
		out[len] = (s << 16) | (eb << 8) | ev;
	}
	for (uint32_t i = threadIdx.x; i < 32768; i += 64) {
		uint32_t s, eb, ev;
		hd::off_slot(i + 1, s, eb, ev);
		out[512 + i] = (s << 24) | (eb << 16) | ev;
	}
}

// The parse publishes 64 positions per step with ONE ds_write_b16; lanes whose four bytes hash alike write the
// same table entry in that instruction.  The encoder (and its CPU twin, which keeps the largest position)
// relies on what gfx950's LDS does then: the highest lane's data stays.  This kernel checks exactly that,
// for 16-bit entries, with conflict patterns from "all lanes on one entry" to "random over 1536 entries".
// (the second half of the blocks does the same with ds_write_b32 on dword entries: the two-way buckets of the lazy levels)
__global__ __launch_bounds__(64) void k_selftest_lds_order(const uint16_t *idx, uint32_t rounds, uint16_t *out)
{
	__shared__ uint16_t table[1536];
	__shared__ uint32_t table32[1536];
	const uint32_t lane = threadIdx.x;
	const bool wide = blockIdx.x >= gridDim.x / 2;
	for (uint32_t r = 0; r < rounds; r++) {
		for (uint32_t i = lane; i < 1536; i += 64) {
			table[i] = 0;
			table32[i] = 0;
		}
		__syncthreads();
		const uint16_t h = idx[(blockIdx.x * rounds + r) * 64 + lane];
		if (wide)
			table32[h] = 0xabcd0000u | (lane + 1);
		else
			table[h] = (uint16_t)(lane + 1);
		__syncthreads();
		out[(blockIdx.x * rounds + r) * 64 + lane] = wide ? (uint16_t)table32[h] : table[h];
	}
}

// The level-1 encoder keeps its token queue in a register and pushes a step's tokens across the lanes (hd::queue_push): the
// k-th token lane's word must arrive in lane (q + k) mod 64 -- the address wraps by itself -- and a lane that has no token
// must not disturb one.  Case c: mask[c] = the token lanes, q[c] = tokens waiting; out = what every lane received
__global__ __launch_bounds__(64) void k_selftest_queue_push(const uint64_t *mask, const uint32_t *q, uint32_t *out)
{
	const uint32_t c = blockIdx.x, lane = threadIdx.x;
	// (in scalar registers, as the encoder has them)
	const uint64_t tm = ((uint64_t)hd::uniform((uint32_t)(mask[c] >> 32)) << 32) | hd::uniform((uint32_t)mask[c]);
	const uint32_t qn = hd::uniform(q[c]);
	out[c * 64 + lane] = hd::queue_push(tm, qn, 0x5a000000u | (c << 8) | lane);
}

// queue_push lets the lanes without a token send as well, to the destination of the first token above them, and leans on
// what ds_permute_b32 does when several lanes send to one: the HIGHEST source lane's data arrives (as the highest lane's
// store stays in k_selftest_lds_order).  Case c: lane l sends its word to lane dst[c * 64 + l] mod 64 (the address is not
// masked: the instruction takes it modulo 64 lanes); out = what every lane received
__global__ __launch_bounds__(64) void k_selftest_permute_order(const uint32_t *dst, uint32_t *out)
{
	const uint32_t c = blockIdx.x, lane = threadIdx.x;
	out[c * 64 + lane] = (uint32_t)__builtin_amdgcn_ds_permute((int)(dst[c * 64 + lane] << 2), (int)(0xa5000000u | (c << 8) | lane));
}

// The step aligns a candidate's bytes with v_alignbyte_b32 and passes the candidate's POSITION as the shift operand: the
// instruction must read bits [1:0] of it and no others.  (In assembly: the compiler must not get to reason about the
// builtin's operand.)  in: a, b, shift per lane; out = ({a, b} >> 8 * shift)[31:0] as the device computes it
__global__ __launch_bounds__(64) void k_selftest_alignbyte(const uint32_t *in, uint32_t *out)
{
	const uint32_t i = blockIdx.x * 64 + threadIdx.x;
	const uint32_t a = in[3 * i], b = in[3 * i + 1], s = in[3 * i + 2];
	uint32_t r;
	asm volatile("v_alignbyte_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(s));
	out[i] = r;
}

// one wavefront per frequency vector through the encoder's Huffman construction
__global__ __launch_bounds__(64) void k_selftest_build(const uint32_t *freq, uint32_t nsyms, uint32_t maxbits, uint8_t *lens)
{
	__shared__ uint32_t f[288], o[288];
	__shared__ hd::HuffScratch hs;
	const uint32_t lane = threadIdx.x;
	for (uint32_t s = lane; s < nsyms; s += 64)
		f[s] = freq[(size_t)blockIdx.x * nsyms + s];
	hd::build_code(f, nsyms, maxbits, o, hs, lane);
	for (uint32_t s = lane; s < nsyms; s += 64)
		lens[(size_t)blockIdx.x * nsyms + s] = (uint8_t)(o[s] >> 16);
}

} // namespace

// ---- LDS write arbitration: of the lanes that store to one entry in one instruction, the highest stays ----
// Kernel == CPU twin (and with it golden hashes and multi-rank determinism) leans on this property of the gfx950 LDS,
// which no document promises: ctx_init() runs this probe once per process and refuses the device if it fails.
// Returns the number of entries that did not hold the highest writer; < 0 on an allocation error.
int hd_probe_lds_order(void)
{
	const uint32_t nb = 16, rounds = 32, n = nb * rounds * 64;
	uint16_t *hx = (uint16_t *)malloc(n * 2), *ho = (uint16_t *)malloc(n * 2), *dx = nullptr, *dout = nullptr;
	uint32_t seed = 777;
	for (uint32_t i = 0; i < n; i++) {
		seed = seed * 1664525u + 1013904223u;
		const uint32_t pat = (i / 64) % 8, l = i % 64;
		// 0: one entry; 1: pairs; 2: two entries alternating; 3: 8 distinct, same bank; 4..7: random over 2^k
		hx[i] = pat == 0 ? 5 : pat == 1 ? (uint16_t)(l / 2) : pat == 2 ? (uint16_t)(l & 1)
			: pat == 3 ? (uint16_t)((l & 7) * 64) : (uint16_t)((seed >> 16) % (pat == 4 ? 4u : pat == 5 ? 16u : pat == 6 ? 64u : 1536u));
	}
	if (hipMalloc((void **)&dx, n * 2) != hipSuccess || hipMalloc((void **)&dout, n * 2) != hipSuccess) {
		free(hx);
		free(ho);
		(void)hipFree(dx);
		return -1;
	}
	(void)hipMemcpy(dx, hx, n * 2, hipMemcpyHostToDevice);
	hipLaunchKernelGGL(k_selftest_lds_order, dim3(nb), dim3(64), 0, 0, dx, rounds, dout);
	int bad = hipMemcpy(ho, dout, n * 2, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
	for (uint32_t g = 0; g < n && !(bad && g == 0); g += 64)
		for (uint32_t l = 0; l < 64; l++) {
			uint32_t top = l;
			for (uint32_t k = l + 1; k < 64; k++)
				if (hx[g + k] == hx[g + l])
					top = k;
			if (ho[g + l] != top + 1) {
				if (bad++ < 5)
					fprintf(stderr, "hipdeflate: LDS store arbitration: group %u lane %u entry %u holds lane %u, "
						"highest writer is %u\n", g / 64, l, hx[g + l], ho[g + l] - 1, top);
			}
		}
	free(hx);
	free(ho);
	(void)hipFree(dx);
	(void)hipFree(dout);
	return bad;
}

// ---- the cross-lane push of the level-1 token queue: every q, masks from empty to full ----
// Every token must arrive at lane (q + k) mod 64 (a lane without a token must not disturb one), and a lane nobody sends to
// reads 0.  Returns the number of cases in which that does not hold; < 0 on an allocation or launch error.
static int hd_probe_queue_push(void)
{
	const uint32_t per_q = 8, nc = 64 * per_q;
	uint64_t *hm = (uint64_t *)malloc(nc * 8), *dm = nullptr;
	uint32_t *hq = (uint32_t *)malloc(nc * 4), *ho = (uint32_t *)malloc(nc * 64 * 4), *dq = nullptr, *dout = nullptr;
	int bad = -1;
	if (hm && hq && ho && hipMalloc((void **)&dm, nc * 8) == hipSuccess && hipMalloc((void **)&dq, nc * 4) == hipSuccess &&
	    hipMalloc((void **)&dout, nc * 64 * 4) == hipSuccess) {
		uint64_t seed = 0x9e3779b97f4a7c15ull;
		for (uint32_t c = 0; c < nc; c++) {
			const uint32_t q = c / per_q, pat = c % per_q;
			seed = seed * 6364136223846793005ull + 1442695040888963407ull;
			const uint64_t r = seed ^ (seed >> 29);
			// 0: every lane; 1: none; 2: one lane; 3: the low q + 1 lanes; 4: every other lane; 5: dense; 6: random; 7: sparse
			hm[c] = pat == 0 ? ~0ull : pat == 1 ? 0ull : pat == 2 ? 1ull << (r >> 58) : pat == 3 ? (q == 63 ? ~0ull : (2ull << q) - 1)
				: pat == 4 ? 0xaaaaaaaaaaaaaaaaull : pat == 5 ? r | (r << 17) | (r >> 23) : pat == 6 ? r : r & (r << 13) & (r >> 7);
			hq[c] = q;
		}
		bool ok = hipMemcpy(dm, hm, nc * 8, hipMemcpyHostToDevice) == hipSuccess &&
			  hipMemcpy(dq, hq, nc * 4, hipMemcpyHostToDevice) == hipSuccess;
		if (ok) {
			hipLaunchKernelGGL(k_selftest_queue_push, dim3(nc), dim3(64), 0, 0, dm, dq, dout);
			ok = hipGetLastError() == hipSuccess && hipMemcpy(ho, dout, nc * 64 * 4, hipMemcpyDeviceToHost) == hipSuccess;
		}
		if (ok) {
			bad = 0;
			for (uint32_t c = 0; c < nc; c++) {
				uint32_t k = 0, wrong = 0;
				// lanes somebody sends to.  (The lanes above the last token send to lane q + count, which is no entry: whatever arrives)
				uint64_t fed = hm[c] >> 63 ? 0ull : 1ull << ((hq[c] + (uint32_t)__builtin_popcountll(hm[c])) & 63);
				for (uint32_t l = 0; l < 64; l++)
					if ((hm[c] >> l) & 1) {
						wrong += ho[c * 64 + ((hq[c] + k) & 63)] != (0x5a000000u | (c << 8) | l);
						fed |= 1ull << ((hq[c] + k) & 63);
						k++;
					}
				for (uint32_t l = 0; l < 64; l++)
					wrong += !((fed >> l) & 1) && ho[c * 64 + l] != 0;
				if (wrong && bad++ < 5)
					fprintf(stderr, "hipdeflate: queue push: q %u mask %016llx: %u lanes of %u tokens not what the queue reads\n",
						hq[c], (unsigned long long)hm[c], wrong, k);
			}
		}
	}
	free(hm);
	free(hq);
	free(ho);
	(void)hipFree(dm);
	(void)hipFree(dq);
	(void)hipFree(dout);
	return bad;
}

// ---- ds_permute_b32 with several senders per destination: the highest source lane's data arrives ----
// queue_push leans on it (hd_device.hpp).  Collisions of 2..64 senders on every destination lane, the sender sets drawn at
// random (the other lanes send elsewhere, colliding as they may), then every lane on one of 2^k destinations at random, with
// address bits above the lane number set.  Every lane must read its highest sender's word, or 0 where nobody sent.
// Returns the number of lanes that read something else; < 0 on an allocation or launch error.
static int hd_probe_permute_order(void)
{
	const uint32_t n_fix = 63 * 64, n_rnd = 7 * 32, nc = n_fix + n_rnd;
	uint32_t *hd = (uint32_t *)malloc(nc * 64 * 4), *ho = (uint32_t *)malloc(nc * 64 * 4), *dd = nullptr, *dout = nullptr;
	int bad = -1;
	if (hd && ho && hipMalloc((void **)&dd, nc * 64 * 4) == hipSuccess && hipMalloc((void **)&dout, nc * 64 * 4) == hipSuccess) {
		uint64_t seed = 0x2545f4914f6cdd1dull;
		auto rnd = [&]() -> uint32_t {
			seed = seed * 6364136223846793005ull + 1442695040888963407ull;
			return (uint32_t)(seed >> 33);
		};
		for (uint32_t c = 0; c < nc; c++) {
			uint32_t *d = hd + c * 64;
			if (c < n_fix) {
				const uint32_t g = 2 + c / 64, to = c % 64;          // g senders on lane `to`
				uint8_t order[64];
				for (uint32_t l = 0; l < 64; l++)
					order[l] = (uint8_t)l;
				for (uint32_t l = 63; l > 0; l--) {                  // a random order of the lanes: its first g send to `to`
					const uint32_t j = rnd() % (l + 1);
					const uint8_t t = order[l];
					order[l] = order[j];
					order[j] = t;
				}
				for (uint32_t k = 0; k < 64; k++)
					d[order[k]] = k < g ? to : (to + 1 + rnd() % 63) & 63;
			} else {
				const uint32_t span = 1u << (1 + (c - n_fix) % 7);       // 2, 4, ..., 64 destinations; then 128: all 64, bit 6 set at random
				for (uint32_t l = 0; l < 64; l++)
					d[l] = rnd() % span + ((c & 1) ? 64u * (rnd() & 0xffff) : 0u);
			}
		}
		bool ok = hipMemcpy(dd, hd, nc * 64 * 4, hipMemcpyHostToDevice) == hipSuccess;
		if (ok) {
			hipLaunchKernelGGL(k_selftest_permute_order, dim3(nc), dim3(64), 0, 0, dd, dout);
			ok = hipGetLastError() == hipSuccess && hipMemcpy(ho, dout, nc * 64 * 4, hipMemcpyDeviceToHost) == hipSuccess;
		}
		if (ok) {
			bad = 0;
			for (uint32_t c = 0; c < nc; c++)
				for (uint32_t l = 0; l < 64; l++) {
					uint32_t want = 0;
					for (uint32_t k = 0; k < 64; k++)
						if ((hd[c * 64 + k] & 63) == l)
							want = 0xa5000000u | (c << 8) | k;       // the highest sender stays
					if (ho[c * 64 + l] != want && bad++ < 5)
						fprintf(stderr, "hipdeflate: ds_permute_b32 collision order: case %u lane %u read %08x, highest sender's word is %08x\n",
							c, l, ho[c * 64 + l], want);
				}
		}
	}
	free(hd);
	free(ho);
	(void)hipFree(dd);
	(void)hipFree(dout);
	return bad;
}

// ---- v_alignbyte_b32 reads bits [1:0] of its shift operand only ----
// Shift operands with every byte offset under: no upper bit, all of them, each upper bit alone, all but each one, and random
// upper bits; against ({a, b} >> 8 * (shift & 3))[31:0].  Returns the number of lanes that differ; < 0 on an error.
static int hd_probe_alignbyte(void)
{
	const uint32_t nb = 2 + 30 + 30 + 66, n = nb * 64;
	uint32_t *hi = (uint32_t *)malloc(n * 12), *ho = (uint32_t *)malloc(n * 4), *din = nullptr, *dout = nullptr;
	int bad = -1;
	if (hi && ho && hipMalloc((void **)&din, n * 12) == hipSuccess && hipMalloc((void **)&dout, n * 4) == hipSuccess) {
		uint64_t seed = 0x9e3779b97f4a7c15ull;
		for (uint32_t i = 0; i < n; i++) {
			const uint32_t blk = i / 64;
			seed = seed * 6364136223846793005ull + 1442695040888963407ull;
			hi[3 * i] = (uint32_t)(seed >> 32);
			hi[3 * i + 1] = (uint32_t)seed * 2654435761u + i;
			seed = seed * 6364136223846793005ull + 1442695040888963407ull;
			const uint32_t up = blk == 0 ? 0u : blk == 1 ? ~3u : blk < 32 ? 4u << (blk - 2) : blk < 62 ? ~3u & ~(4u << (blk - 32))
					  : (uint32_t)(seed >> 32) & ~3u;
			hi[3 * i + 2] = up | (i & 3);
		}
		bool ok = hipMemcpy(din, hi, n * 12, hipMemcpyHostToDevice) == hipSuccess;
		if (ok) {
			hipLaunchKernelGGL(k_selftest_alignbyte, dim3(nb), dim3(64), 0, 0, din, dout);
			ok = hipGetLastError() == hipSuccess && hipMemcpy(ho, dout, n * 4, hipMemcpyDeviceToHost) == hipSuccess;
		}
		if (ok) {
			bad = 0;
			for (uint32_t i = 0; i < n; i++) {
				const uint64_t wide = ((uint64_t)hi[3 * i] << 32) | hi[3 * i + 1];
				const uint32_t want = (uint32_t)(wide >> (8 * (hi[3 * i + 2] & 3)));
				if (ho[i] != want && bad++ < 5)
					fprintf(stderr, "hipdeflate: v_alignbyte_b32 {%08x, %08x} by %08x gave %08x, want %08x\n",
						hi[3 * i], hi[3 * i + 1], hi[3 * i + 2], ho[i], want);
			}
		}
	}
	free(hi);
	free(ho);
	(void)hipFree(din);
	(void)hipFree(dout);
	return bad;
}

/* test entry: code lengths the DEVICE Huffman construction gives `nvec` frequency vectors of `nsyms` symbols
 * each (tests/test_gpu_parity.py compares them with the oracle's on adversarial distributions) */
extern "C" int hipdeflate_test_build_lengths(const uint32_t *freq, uint32_t nvec, uint32_t nsyms, uint32_t maxbits,
					     uint8_t *lens_out)
{
	int r = hipdeflate_available();
	if (r)
		return r;
	// no length-limited code exists for more than 2^maxbits symbols (the builder's push-up loop would run off
	// its length counters)
	if (!freq || !lens_out || !nvec || nsyms < 2 || nsyms > 288 || maxbits < 1 || maxbits > 15 || nsyms > (1u << maxbits))
		return HD_E_ARG;
	uint32_t *df = nullptr;
	uint8_t *dl = nullptr;
	const size_t n = (size_t)nvec * nsyms;
	if (hipMalloc((void **)&df, n * 4) != hipSuccess)
		return HD_E_NOMEM;
	if (hipMalloc((void **)&dl, n) != hipSuccess) {
		(void)hipFree(df);
		return HD_E_NOMEM;
	}
	(void)hipMemcpy(df, freq, n * 4, hipMemcpyHostToDevice);
	hipLaunchKernelGGL(k_selftest_build, dim3(nvec), dim3(64), 0, 0, df, nsyms, maxbits, dl);
	const hipError_t e = hipMemcpy(lens_out, dl, n, hipMemcpyDeviceToHost);
	(void)hipFree(df);
	(void)hipFree(dl);
	return e == hipSuccess ? 0 : HD_E_NODEVICE;
}

extern "C" int hipdeflate_selftest(void)
{
	int r = hipdeflate_available();
	if (r)
		return r;
	int fails = 0;
	// ---- scan -------------------------------------------------------------
	{
		const int nb = 8;
		uint32_t hx[nb * 64], hi[nb * 64];
		uint32_t seed = 12345;
		for (int i = 0; i < nb * 64; i++) {
			seed = seed * 1664525u + 1013904223u;
			hx[i] = i < 64 ? 31 : i < 128 ? (i & 1) : (seed >> 27);
		}
		uint32_t *dx, *di;
		if (hipMalloc((void **)&dx, sizeof(hx)) != hipSuccess || hipMalloc((void **)&di, sizeof(hi)) != hipSuccess)
			return HD_E_NOMEM;
		(void)hipMemcpy(dx, hx, sizeof(hx), hipMemcpyHostToDevice);
		hipLaunchKernelGGL(k_selftest_scan, dim3(nb), dim3(64), 0, 0, dx, di);
		(void)hipMemcpy(hi, di, sizeof(hi), hipMemcpyDeviceToHost);
		for (int b = 0; b < nb; b++) {
			uint32_t run = 0;
			for (int l = 0; l < 64; l++) {
				run += hx[b * 64 + l];
				if (hi[b * 64 + l] != run) {
					if (fails < 5)
						fprintf(stderr, "hipdeflate selftest: scan[%d][%d] = %u, want %u\n", b, l,
							hi[b * 64 + l], run);
					fails++;
				}
			}
		}
		(void)hipFree(dx);
		(void)hipFree(di);
	}
	// ---- LDS write arbitration (also run by ctx_init) ----------------------------
	{
		const int bad = hd_probe_lds_order();
		if (bad < 0)
			return HD_E_NOMEM;
		fails += bad;
	}
	// ---- the level-1 token queue's cross-lane push ----------------------------------
	{
		const int bad = hd_probe_queue_push();
		if (bad < 0)
			return HD_E_NOMEM;
		fails += bad;
	}
	// ---- ... and the collision order of ds_permute_b32 it leans on --------------------------------
	{
		const int bad = hd_probe_permute_order();
		if (bad < 0)
			return HD_E_NOMEM;
		fails += bad;
	}
	// ---- the shift operand of v_alignbyte_b32 (the level-1 and level-2 step) --------------------------
	{
		const int bad = hd_probe_alignbyte();
		if (bad < 0)
			return HD_E_NOMEM;
		fails += bad;
	}
	// ---- slot arithmetic vs RFC 1951 3.2.5 tables ---------------------------
	{
		static const uint16_t lbase[29] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59,
						    67, 83, 99, 115, 131, 163, 195, 227, 258 };
		static const uint8_t lext[29] = { 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3,
						  4, 4, 4, 4, 5, 5, 5, 5, 0 };
		static const uint16_t obase[30] = { 1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513,
						    769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577 };
		static const uint8_t oext[30] = { 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8,
						  9, 9, 10, 10, 11, 11, 12, 12, 13, 13 };
		const size_t n = 512 + 32768;
		uint32_t *d, *h = (uint32_t *)malloc(n * 4);
		if (hipMalloc((void **)&d, n * 4) != hipSuccess)
			return HD_E_NOMEM;
		hipLaunchKernelGGL(k_selftest_slots, dim3(1), dim3(64), 0, 0, d);
		(void)hipMemcpy(h, d, n * 4, hipMemcpyDeviceToHost);
		for (uint32_t len = 3; len <= 258; len++) {
			uint32_t s = h[len] >> 16, eb = (h[len] >> 8) & 0xff, ev = h[len] & 0xff;
			// 258 is symbol 285 (index 28), never 284 + extra 31
			if (s > 28 || lext[s] != eb || lbase[s] + ev != len || ev >= (1u << eb) + (eb == 0) ||
			    (len == 258 && s != 28))
				fails++;
		}
		for (uint32_t i = 0; i < 32768; i++) {
			uint32_t s = h[512 + i] >> 24, eb = (h[512 + i] >> 16) & 0xff, ev = h[512 + i] & 0xffff;
			if (s > 29 || oext[s] != eb || obase[s] + ev != i + 1 || (eb && ev >= (1u << eb)))
				fails++;
		}
		if (fails)
			fprintf(stderr, "hipdeflate selftest: slot arithmetic failures so far: %d\n", fails);
		free(h);
		(void)hipFree(d);
	}
	// ---- CRC folding: through the public inflate/deflate entry points -------
	{
		// stored level-0 members of assorted sizes carry the kernel's CRC-32;
		// compare with a bitwise CRC computed here
		const uint32_t sizes[] = { 0, 1, 15, 16, 17, 1023, 1024, 1025, 4096 + 7, 65280, 65536, 70001 };
		for (uint32_t n : sizes) {
			uint8_t *src = (uint8_t *)malloc(n + 1), *dst = (uint8_t *)malloc(n + 1024);
			uint32_t seed = n * 2654435761u + 1;
			for (uint32_t i = 0; i < n; i++) {
				seed = seed * 1664525u + 1013904223u;
				src[i] = seed >> 24;
			}
			uint32_t c = 0xffffffffu;
			for (uint32_t i = 0; i < n; i++) {
				c ^= src[i];
				for (int k = 0; k < 8; k++)
					c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
			}
			c = ~c;
			uint64_t off = 0;
			uint32_t len = n, olen = 0, crc = 0;
			int32_t st = -1;
			int rr = hipdeflate_batch_deflate(src, &off, &len, 1, 0, HD_FRAME_RAW, dst, (n + 1024) & ~15u, n + 1000,
							  &olen, &crc, &st);
			if (rr || st || crc != c) {
				fprintf(stderr, "hipdeflate selftest: crc n=%u got %08x want %08x (rc %d st %d)\n", n, crc, c,
					rr, st);
				fails++;
			}
			free(src);
			free(dst);
		}
	}
	return fails ? 1 : 0;
}
