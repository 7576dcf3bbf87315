// count_kernels.h -- kmx_count_*: the canonical k-mer of every counted window of a batch of sequences.
// Included at the end of kernels.hip (after range_kernels.h): it uses seq_off / seq_upper / seq_code of the
// query-along-sequences section, so the window rule and the sequence boundaries are those of kmx_query_seqs.
//
// The counting rule (include/kmx.h): a window is counted when it lies wholly inside one sequence and its k bytes are all
// bases, A C G T or a c g t (A=0 C=1 G=2 T=3, CKmerAPI::num_codes, kmc_api/kmer_api.h:264-275); its key is the numeric minimum
// of the 2k-bit forward word and its reverse complement.  Sorting, run-length encoding and merging the keys happen in
// count_device.hip.

// the 2-bit code of a base, either case; 4 = not a base (N, IUPAC letters, anything else)
// (clearing bit 5 maps a c g t, and only them, onto A C G T)
__device__ __forceinline__ u32 count_code(u32 c) { return seq_code(c & ~0x20u); }

static constexpr int CNT_BT = 256;
static constexpr int CNT_RUN = 16;                                  // consecutive windows rolled by one lane
static constexpr int CNT_WIN = CNT_BT * CNT_RUN;                   // windows per block
static constexpr int CNT_TILE = CNT_WIN + 64;                      // + the k - 1 <= 63 bases of the block's last window

// windows [p0, p0 + n_win) (all < n_bases).  Every lane rolls the forward and reverse-complement words over CNT_RUN
// consecutive windows: k - 1 bases of prologue, then one base per window; a non-base byte or a sequence boundary restarts
// the roll.  A lane keeps its keys in registers and a wave reserves room for all of them with one atomic: keys[o] for
// o < cap (W = 1: key_lo only; W = 2: key_hi = the high word, key_lo = the low word).  *cnt advances by the windows
// counted, also past cap (the host sizes cap to the windows it launches, so it never gets there).  Offsets are clamped
// where they are read (seq_off), so no offsets move a read outside seq[0, n_bases) or offs[0, n_seqs].
template <int W> __global__ __launch_bounds__(CNT_BT) void k_count_windows(int k, const unsigned char *seq, u64 n_bases, const u64 *offs, u64 n_seqs, u64 p0, u64 n_win, u64 *key_lo, u64 *key_hi, u64 cap, unsigned long long *cnt)
{
	__shared__ unsigned char s_code[CNT_TILE];
	__shared__ u64 s_u[2];
	const int tid = threadIdx.x, lane = tid & 63;
	const u64 t0 = p0 + (u64)blockIdx.x * CNT_WIN, p_end = p0 + n_win;
	const u64 t_last = (t0 + CNT_WIN < p_end ? t0 + CNT_WIN : p_end) - 1;
	const u64 b_end = t0 + CNT_WIN + k - 1 < n_bases ? t0 + CNT_WIN + k - 1 : n_bases;   // the bases this block reads: [t0, b_end)
	if (tid == 0) s_u[0] = seq_upper(offs, 0, n_seqs + 1, t0, n_bases);
	if (tid == 64) s_u[1] = seq_upper(offs, 0, n_seqs + 1, t_last, n_bases);
	const unsigned char *src = seq + t0;
	const int nb = (int)(b_end - t0);
	if (((uintptr_t)src & 3) == 0) {
		for (int j = 4 * tid; j < nb; j += 4 * CNT_BT) {
			if (j + 4 <= nb) {
				const u32 w = *(const u32 *)(src + j);
#pragma unroll
				for (int q = 0; q < 4; q++) s_code[j + q] = (unsigned char)count_code((w >> (8 * q)) & 0xFFu);
			} else
				for (int q = j; q < nb; q++) s_code[q] = (unsigned char)count_code(src[q]);
		}
	} else
		for (int j = tid; j < nb; j += CNT_BT) s_code[j] = (unsigned char)count_code(src[j]);
	__syncthreads();

	const u64 q0 = t0 + (u64)tid * CNT_RUN;                          // this lane's first window
	u32 valid = 0;                                                   // bit r: window q0 + r is counted
	u64 v_lo[CNT_RUN], v_hi[CNT_RUN];
	if (q0 < p_end) {
		const u64 u0 = s_u[0], u1 = s_u[1];
		u64 u = seq_upper(offs, u0, u1 > u0 ? u1 : u0, q0, n_bases);  // sequence u - 1 holds q0 (when 1 <= u <= n_seqs)
		bool in_seq = u >= 1 && u <= n_seqs && seq_off(offs, u - 1, n_bases) <= q0;
		u64 nxt = u <= n_seqs ? seq_off(offs, u, n_bases) : ~0ULL;   // where the next sequence starts
		const u64 lmask = k >= 32 ? ~0ULL : (1ULL << (2 * (k & 31))) - 1;
		const u64 hmask = k == 64 ? ~0ULL : (k > 32 ? (1ULL << (2 * k - 64)) - 1 : 0);
		const int rsh = W == 1 ? 2 * k - 2 : 2 * k - 66;
		u64 f_lo = 0, f_hi = 0, r_lo = 0, r_hi = 0;
		int len = 0;                                                 // bases of the current run, up to k
		auto step = [&](u64 j) {
			while (u <= n_seqs && nxt <= j) {                        // j starts a later sequence
				u++;
				nxt = u <= n_seqs ? seq_off(offs, u, n_bases) : ~0ULL;
				in_seq = u <= n_seqs;
				len = 0;
			}
			const u32 c = (j < b_end && in_seq) ? (u32)s_code[j - t0] : 4u;
			if (c > 3u) { len = 0; return; }
			if (W == 1) {
				f_lo = ((f_lo << 2) | c) & lmask;
				r_lo = (r_lo >> 2) | ((u64)(3u - c) << rsh);
			} else {
				f_hi = ((f_hi << 2) | (f_lo >> 62)) & hmask;
				f_lo = (f_lo << 2) | c;
				r_lo = (r_lo >> 2) | (r_hi << 62);
				r_hi = (r_hi >> 2) | ((u64)(3u - c) << rsh);
			}
			len = len < k ? len + 1 : k;
		};
		for (int i = 0; i < k - 1; i++) step(q0 + (u64)i);
#pragma unroll
		for (int r = 0; r < CNT_RUN; r++) {
			step(q0 + (u64)(k - 1 + r));
			if (len >= k && q0 + r < p_end) {
				valid |= 1u << r;
				const bool fwd = W == 1 ? f_lo <= r_lo : (f_hi < r_hi || (f_hi == r_hi && f_lo <= r_lo));
				v_lo[r] = fwd ? f_lo : r_lo;
				v_hi[r] = fwd ? f_hi : r_hi;
			}
		}
	}
	// room for the wave's keys: an inclusive scan of the lanes' counts, one atomic
	const u32 nv = (u32)__popc(valid);
	u32 incl = nv;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const u32 t = __shfl_up(incl, d, 64);
		if (lane >= d) incl += t;
	}
	const u32 tot = __shfl(incl, 63, 64);
	unsigned long long base = 0;
	if (lane == 63 && tot) base = atomicAdd(cnt, (unsigned long long)tot);
	base = __shfl(base, 63, 64);
	u64 o = base + incl - nv;
#pragma unroll
	for (int r = 0; r < CNT_RUN; r++)
		if ((valid >> r) & 1u) {
			if (o < cap) {
				key_lo[o] = v_lo[r];
				if (W == 2) key_hi[o] = v_hi[r];
			}
			o++;
		}
}

namespace kmxk {

// the windows [p0, p0 + n_win) of the sequences -> the keys of the counted ones, appended at *cnt (see k_count_windows)
void count_windows(int k, const unsigned char *seq, u64 n_bases, const u64 *offs, u64 n_seqs, u64 p0, u64 n_win, u64 *key_lo, u64 *key_hi, u64 cap, unsigned long long *cnt, hipStream_t st)
{
	if (!n_win) return;
	const unsigned grid = (unsigned)((n_win + CNT_WIN - 1) / CNT_WIN);
	DISPATCH_W((k + 31) / 32, hipLaunchKernelGGL(k_count_windows<W>, dim3(grid), dim3(CNT_BT), 0, st, k, seq, n_bases, offs, n_seqs, p0, n_win, key_lo, key_hi, cap, cnt));
}

}   // namespace kmxk
