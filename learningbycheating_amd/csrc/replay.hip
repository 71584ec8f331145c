// Device-resident prioritised replay buffer of phase 2 (DAgger; reference training/phase2_utils.py:190-289 ReplayBuffer and
// weighted_random_choice, :219-227): what the reference does per sample on the host -- a weighted draw over up to 100,000 loss
// weights, the gather of the drawn frames, np.repeat for --batch_aug, the write-back of the new weights -- as kernels over whole
// batches, so that a training step has no host round trip.
//   cdf        weights f32 [n] -> inclusive prefix sum in double [n] (+ the count of weights that are negative, NaN or infinite; those
//              contribute 0).  Three passes: in-tile scan (1024 weights per workgroup), scan of the tile totals by one workgroup,
//              add.  No workspace: a tile's total lives in its last cdf slot, pass 2 turns exactly those slots into their final
//              values, pass 3 adds the previous tile's (final) last slot to every other slot of the tile.  No atomics: the order of
//              every sum is fixed, the result is the same on every run.  Runs once per epoch.
//              Rounding: with weights whose sums are exact in double (the tests' small integers) the result IS the sequential sum.
//              With real losses every slot is a correctly ordered sum rounded at a few points; inside one lane's four weights and
//              across a tile's end the values never step back, but where one lane's run meets the next (every fourth slot) the two
//              neighbours are rounded along different paths and may differ by one unit in the last place of a double either way.
//   sample     draw j of step t: u = 53 random bits of hash3(seed ^ t_hi, 2j | 2j + 1, t_lo) scaled to [0, cdf[n-1]); the index is
//              the first i with cdf[i] > u (np.searchsorted(cdf, u, side="right")): an entry of weight 0 has cdf[i] == cdf[i-1] and
//              is never the first one above u.  (That equality is exact wherever the sums are; by the rounding note above a zero
//              weight in a lane's first slot can own an interval of one unit in the last place, relative width 2^-53 of the total:
//              less than one draw in 10^15.)
//   gather     dst row r = src row idx[r / reps] (repeat_interleave), 16 bytes per lane; scatter: dst row slot[m] = src row m.
//              gather_indirect: dst row r = src row frame_of_slot[idx[r / reps]] -- a buffer that holds frame INDICES into a resident
//              dataset gathers straight from that dataset's frames.
//   meta       speed[idx] and one_hot(cmd[idx]) with the same fan-out.
//   writeback  new_w[idx[b]] = mean of the reps weights of source sample b; of equal indices the LAST b wins (numpy fancy assignment).
//   admit      m scored candidates (frame index, cmd, speed, weight) into a buffer of n occupied slots out of `limit` that holds frame
//              indices: what m ReplayBuffer.add_data calls decide (phase2_utils.py:256-265), in one launch of ONE workgroup and with
//              ties made definite.  key(w) = w if finite and >= 0, else -1.  (1) a candidate whose frame is stored refreshes that
//              slot's weight; (2) the others fill the free slots in candidate order; (3) when candidates are still waiting the buffer
//              is full: stored slots and waiting candidates are ranked by key descending -- stored before waiting, lower index first --
//              the first `limit` stay, and the evicted slots in ascending order take the surviving candidates in candidate order.
//              The rank is never materialised: the key of rank `limit` is found bit by bit (31 counting passes over the keys as
//              ordered unsigned integers), of the entries AT that key the first ones in rank order stay (one scan), the evicted slots
//              and the survivors are numbered by two more scans.  Every scan gives a thread one contiguous run of entries and adds
//              the runs' counts in thread order: no atomics, the result is a function of the inputs.  Runs once per episode.
#include "lbc_common.hpp"
#include "lbc_hash.hpp"
#include "lbc_kernels.hpp"

namespace {

constexpr int kCdfThreads = 256;
constexpr int kCdfPerThread = 4;
constexpr int kCdfTile = kCdfThreads * kCdfPerThread;

// a weight the sampler can use: finite and >= 0 (NaN fails both comparisons)
__device__ __forceinline__ bool weight_ok(float w) { return w >= 0.f && w <= 3.402823466e38f; }

// inclusive scan of one value per thread over the workgroup (Hillis-Steele on two LDS planes); buf: 2 * blockDim.x values
template <typename T>
__device__ __forceinline__ T block_scan_inclusive(T v, T* buf)
{
    const int t = (int)threadIdx.x, nt = (int)blockDim.x;
    int cur = 0;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < nt; d <<= 1) {
        const T x = buf[cur * nt + t] + (t >= d ? buf[cur * nt + t - d] : T(0));
        buf[(cur ^ 1) * nt + t] = x;
        cur ^= 1;
        __syncthreads();
    }
    const T r = buf[cur * nt + t];
    __syncthreads();                 // (the caller may reuse buf)
    return r;
}

// pass 1: cdf[i] = sum of the usable weights of i's tile up to and including i
__global__ __launch_bounds__(kCdfThreads) void cdf_tile_scan_k(const float* __restrict__ w, int n, double* __restrict__ cdf)
{
    __shared__ double buf[2 * kCdfThreads];
    const long long base = (long long)blockIdx.x * kCdfTile + (long long)threadIdx.x * kCdfPerThread;
    double v[kCdfPerThread];
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < kCdfPerThread; ++k) {
        const long long i = base + k;
        const float x = i < n ? w[i] : 0.f;
        sum += weight_ok(x) ? (double)x : 0.0;
        v[k] = sum;
    }
    const double before = block_scan_inclusive(sum, buf) - sum;
#pragma unroll
    for (int k = 0; k < kCdfPerThread; ++k) {
        const long long i = base + k;
        if (i < n) cdf[i] = before + v[k];
    }
}

// pass 2 (one workgroup): the last slot of every tile becomes its final value; the unusable weights are counted.  The totals are chained
// in tile order by one thread (in LDS, 1024 at a time): final[b] = final[b - 1] + total[b] is then the SAME expression pass 3 evaluates
// for every other slot of tile b (final[b - 1] + local), so the sums do not step back across a tile's end.
__global__ __launch_bounds__(1024) void cdf_tile_totals_k(const float* __restrict__ w, int n, double* __restrict__ cdf, long long* __restrict__ bad_count)
{
    __shared__ double buf[1024];
    __shared__ int bad[1024];
    const int t = (int)threadIdx.x, nt = (int)blockDim.x;
    const int tiles = (int)(((long long)n + kCdfTile - 1) / kCdfTile);
    double carry = 0.0;                                  // (thread 0's copy is the one that counts)
    for (int t0 = 0; t0 < tiles; t0 += nt) {
        const int tile = t0 + t;
        long long last = ((long long)tile + 1) * kCdfTile - 1;
        if (last > (long long)n - 1) last = (long long)n - 1;
        buf[t] = tile < tiles ? cdf[last] : 0.0;
        __syncthreads();
        if (t == 0) {
            const int m = tiles - t0 < nt ? tiles - t0 : nt;
            for (int k = 0; k < m; ++k) { carry += buf[k]; buf[k] = carry; }
        }
        __syncthreads();
        if (tile < tiles) cdf[last] = buf[t];
        __syncthreads();
    }
    int c = 0;
    for (long long i = t; i < n; i += nt) c += weight_ok(w[i]) ? 0 : 1;
    bad[t] = c;
    __syncthreads();
    if (t == 0) {
        long long s = 0;
        for (int k = 0; k < nt; ++k) s += bad[k];
        *bad_count = s;
    }
}

// pass 3: every slot of tile b > 0 but its last gets the final value of tile b - 1's last slot added
__global__ __launch_bounds__(kCdfThreads) void cdf_tile_add_k(int n, double* __restrict__ cdf)
{
    const long long tile = (long long)blockIdx.x + 1;
    long long last = (tile + 1) * kCdfTile - 1;
    if (last > (long long)n - 1) last = (long long)n - 1;
    const double off = cdf[tile * kCdfTile - 1];
    for (long long i = tile * kCdfTile + threadIdx.x; i < last; i += kCdfThreads) cdf[i] += off;
}

__global__ __launch_bounds__(256) void sample_k(const double* __restrict__ cdf, int n, unsigned seed, unsigned t_lo, unsigned t_hi, int B,
                                                int* __restrict__ idx)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= B) return;
    const double total = cdf[n - 1];
    const unsigned h1 = hash3(seed ^ t_hi, 2u * (unsigned)j, t_lo), h2 = hash3(seed ^ t_hi, 2u * (unsigned)j + 1u, t_lo);
    // 27 + 26 = 53 bits: exact in a double, u01 in [0, 1); one rounding in the product with the total
    const double u01 = ((double)(h1 >> 5) * 67108864.0 + (double)(h2 >> 6)) * (1.0 / 9007199254740992.0);
    const double u = u01 * total;
    int lo = 0, hi = n;                              // first i with cdf[i] > u
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > u) hi = mid; else lo = mid + 1;
    }
    if (lo >= n) {                                   // the product rounded up to the total: the last entry of non-zero weight,
        lo = 0; hi = n - 1;                          // = the first i with cdf[i] >= total
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (cdf[mid] >= total) hi = mid; else lo = mid + 1;
        }
    }
    idx[j] = lo;
}

// Row copy through an index, 16 bytes per lane, U chunks in flight per lane.  Workgroup (x, y): chunks [x * 256 * U, ...) of the rows
// y, y + gridDim.y, ...  GATHER: dst row r <- src row idx[r / reps]; else (scatter): dst row idx[r] <- src row r.  INDIRECT: the index
// is looked up once more, in `via` (gather_indirect: src row via[idx[r / reps]]).
template <int U, bool GATHER, bool INDIRECT>
__global__ __launch_bounds__(256) void row_copy_k(const uint4* __restrict__ src, uint4* __restrict__ dst, const int* __restrict__ idx, long long rows,
                                                  int reps, long long chunks_per_row, const int* __restrict__ via)
{
    const long long c0 = (long long)blockIdx.x * (256 * U) + threadIdx.x;
    for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
        long long other = (long long)idx[GATHER ? r / reps : r];
        if (INDIRECT) other = (long long)via[other];
        const uint4* s = src + (GATHER ? other : r) * chunks_per_row;
        uint4* d = dst + (GATHER ? r : other) * chunks_per_row;
        if ((long long)(blockIdx.x + 1) * (256 * U) <= chunks_per_row) {       // a whole span: U loads in flight, then U stores
            uint4 v[U];
#pragma unroll
            for (int k = 0; k < U; ++k) v[k] = s[c0 + k * 256];
#pragma unroll
            for (int k = 0; k < U; ++k) d[c0 + k * 256] = v[k];
        } else {                                                               // the row's last span
            for (long long c = c0; c < chunks_per_row; c += 256) d[c] = s[c];
        }
    }
}

__global__ __launch_bounds__(256) void meta_k(const float* __restrict__ speed, const int* __restrict__ cmd, const int* __restrict__ idx, int rows, int reps,
                                              float* __restrict__ speed_out, float* __restrict__ onehot_out)
{
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= rows) return;
    const int i = idx[r / reps];
    speed_out[r] = speed[i];
    int c = cmd[i] - 1;                              // train_utils.one_hot: clamp(cmd - 1, 0, 3)
    c = c < 0 ? 0 : (c > 3 ? 3 : c);
#pragma unroll
    for (int k = 0; k < 4; ++k) onehot_out[(long long)r * 4 + k] = k == c ? 1.f : 0.f;
}

// one workgroup, thread b = source sample b: writes unless a later sample carries the same index
__global__ __launch_bounds__(1024) void writeback_k(const float* __restrict__ w_batch, const int* __restrict__ idx, int B, int reps, int n,
                                                    float* __restrict__ new_w)
{
    __shared__ int sidx[1024];
    const int b = (int)threadIdx.x;
    const int i = b < B ? idx[b] : -1;
    sidx[b] = i;
    __syncthreads();
    if (i < 0 || i >= n) return;
    for (int k = b + 1; k < B; ++k)
        if (sidx[k] == i) return;
    float s = 0.f;
    for (int k = 0; k < reps; ++k) s += w_batch[(long long)b * reps + k];
    new_w[i] = s / (float)reps;
}

// ---- admit ------------------------------------------------------------------------------------------------------------
constexpr int kAdmitThreads = 1024;
constexpr int kAdmitMax = 1 << 20;                   // slots and candidates per call: a thread's run stays below 1,025 entries

// key(w) as an unsigned integer of the same order: unusable weights (key -1) -> 1, w >= 0 -> its bit pattern + 2 (non-negative floats
// order as their bits; -0.0 counts as 0.0).  0 is left for "takes no part in the ranking".  The largest value is 0x7f800001 < 2^31.
__device__ __forceinline__ unsigned admit_key(float w)
{
    return weight_ok(w) ? (__builtin_bit_cast(unsigned, w) & 0x7fffffffu) + 2u : 1u;
}

// sum of one int per thread over the workgroup, handed to every thread; blockDim.x is a power of two; buf: blockDim.x ints
__device__ __forceinline__ int block_sum(int v, int* buf)
{
    const int t = (int)threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int d = (int)blockDim.x >> 1; d > 0; d >>= 1) {
        if (t < d) buf[t] += buf[t + d];
        __syncthreads();
    }
    const int r = buf[0];
    __syncthreads();
    return r;
}

// The entries [0, N) in index order, one contiguous run per thread: emit(i, r, p) with p = pred(i) and r = the number of entries before i
// for which pred holds.  pred is evaluated twice per entry and must not depend on what emit writes.  -> the number of entries for which
// pred holds, in every thread.  buf: 2 * blockDim.x ints.
template <class Pred, class Emit>
__device__ __forceinline__ int block_number(int N, int* buf, Pred pred, Emit emit)
{
    const int t = (int)threadIdx.x, nt = (int)blockDim.x;
    const int per = (N + nt - 1) / nt;
    const int i0 = t * per < N ? t * per : N, i1 = i0 + per < N ? i0 + per : N;
    int c = 0;
    for (int i = i0; i < i1; ++i) c += pred(i) ? 1 : 0;
    const int incl = block_scan_inclusive(c, buf);
    int r = incl - c;
    for (int i = i0; i < i1; ++i) {
        const bool p = pred(i);
        emit(i, r, p);
        r += p ? 1 : 0;
    }
    if (t == nt - 1) buf[0] = incl;
    __syncthreads();
    const int total = buf[0];
    __syncthreads();
    return total;
}

// One workgroup.  ukey [limit + m], rank [m], evslot [m]: workspace.  Every branch around a barrier is uniform (it depends on counts that
// every thread holds), and a barrier stands between every write of an array and the reads of it by other threads.
// (No __restrict__ on what the kernel writes: threads hand values to each other through these arrays.)
__global__ __launch_bounds__(kAdmitThreads) void admit_k(float* weights, int* frame, int* cmd, float* speed, int* slot_of_frame, int n, int limit,
                                                         const float* __restrict__ cw, const int* __restrict__ cframe, const int* __restrict__ ccmd,
                                                         const float* __restrict__ cspeed, int m, unsigned* ukey, int* rank, int* evslot, int* record)
{
    __shared__ int buf[2 * kAdmitThreads];
    const int t = (int)threadIdx.x, nt = (int)blockDim.x;
    // 1. refresh: a stored frame takes the candidate's weight; the others are numbered in candidate order
    const int waiting = block_number(m, buf, [&](int j) { return slot_of_frame[cframe[j]] < 0; },
                                     [&](int j, int r, bool wait) {
                                         rank[j] = wait ? r : -1;
                                         if (!wait) weights[slot_of_frame[cframe[j]]] = cw[j];
                                     });
    // 2. append: the first `room` of them into the free slots
    const int room = limit - n < waiting ? limit - n : waiting;
    for (int j = t; j < m; j += nt) {
        const int r = rank[j];
        if (r >= 0 && r < room) {
            const int s = n + r;
            weights[s] = cw[j]; frame[s] = cframe[j]; cmd[s] = ccmd[j]; speed[s] = cspeed[j];
            slot_of_frame[cframe[j]] = s;
        }
    }
    int n_after = n + room, admitted = room, evicted = 0;
    if (waiting > room) {                            // 3. compete: the buffer is full, waiting - room candidates stand outside
        __syncthreads();
        const int T = limit + m;
        for (int i = t; i < limit; i += nt) ukey[i] = admit_key(weights[i]);
        for (int j = t; j < m; j += nt) ukey[limit + j] = rank[j] >= room ? admit_key(cw[j]) : 0u;
        __syncthreads();
        // the key of rank `limit`: the largest value that at least `limit` entries reach (1 is reached by all that take part)
        unsigned thr = 0;
        for (int bit = 30; bit >= 0; --bit) {
            const unsigned probe = thr | (1u << bit);
            int c = 0;
            for (int i = t; i < T; i += nt) c += ukey[i] >= probe ? 1 : 0;
            if (block_sum(c, buf) >= limit) thr = probe;
        }
        int c = 0;
        for (int i = t; i < T; i += nt) c += ukey[i] > thr ? 1 : 0;
        const int ties = limit - block_sum(c, buf);  // of the entries AT the key, the first `ties` in rank order (= index order) stay
        block_number(T, buf, [&](int i) { return ukey[i] == thr; },
                     [&](int i, int r, bool at) { ukey[i] = (ukey[i] > thr || (at && r < ties)) ? 1u : 0u; });      // ukey: 1 = stays
        // evicted slots in ascending order; their frames leave the map (before any survivor overwrites frame[])
        int old = 0;
        const int gone = block_number(limit, buf, [&](int i) { return ukey[i] == 0u; },
                                      [&](int i, int r, bool out) {
                                          if (out) {
                                              evslot[r] = i;
                                              slot_of_frame[frame[i]] = -1;
                                              old += i < n ? 1 : 0;
                                          }
                                      });
        evicted = block_sum(old, buf);
        // surviving candidates in candidate order take them
        const int survivors = block_number(m, buf, [&](int j) { return ukey[limit + j] == 1u; },
                                           [&](int j, int r, bool in) {
                                               if (in) {
                                                   const int s = evslot[r];
                                                   weights[s] = cw[j]; frame[s] = cframe[j]; cmd[s] = ccmd[j]; speed[s] = cspeed[j];
                                                   slot_of_frame[cframe[j]] = s;
                                               }
                                           });
        admitted = room + survivors - (gone - evicted);
    }
    if (t == 0) {
        record[0] = n_after; record[1] = m - waiting; record[2] = admitted; record[3] = evicted;
    }
}

template <bool GATHER, bool INDIRECT = false>
int row_copy_launch(const unsigned char* src, unsigned char* dst, const int* idx, long long rows, int reps, long long row_bytes, hipStream_t s,
                    const int* via = nullptr)
{
    const long long cpr = row_bytes / 16;
    // 16 KB per workgroup once that still yields a thousand workgroups, 4 KB below (a batch of 4 frames: 180 instead of 48)
    const bool wide = rows * cpr >= 1024LL * 1024;
    const long long per = wide ? 1024 : 256;
    const dim3 grid((unsigned)((cpr + per - 1) / per), (unsigned)(rows < 65535 ? rows : 65535));
    if (wide)
        hipLaunchKernelGGL((row_copy_k<4, GATHER, INDIRECT>), grid, dim3(256), 0, s, reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), idx, rows,
                           reps, cpr, via);
    else
        hipLaunchKernelGGL((row_copy_k<1, GATHER, INDIRECT>), grid, dim3(256), 0, s, reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), idx, rows,
                           reps, cpr, via);
    return LBC_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int lbc_replay_cdf_launch(const float* w, int n, double* cdf, long long* bad_count, hipStream_t s)
{
    LBC_REQUIRE(w && cdf && bad_count, "replay_cdf: null argument");
    LBC_REQUIRE(n >= 1, "replay_cdf: n = %d, need at least one weight", n);
    const int tiles = (int)(((long long)n + kCdfTile - 1) / kCdfTile);
    LbcProfScope prof("replay_cdf", 0.0, 20.0 * n, s);
    hipLaunchKernelGGL(cdf_tile_scan_k, dim3((unsigned)tiles), dim3(kCdfThreads), 0, s, w, n, cdf);
    hipLaunchKernelGGL(cdf_tile_totals_k, dim3(1), dim3(1024), 0, s, w, n, cdf, bad_count);
    if (tiles > 1) hipLaunchKernelGGL(cdf_tile_add_k, dim3((unsigned)(tiles - 1)), dim3(kCdfThreads), 0, s, n, cdf);
    return lbc_check_launch("replay_cdf");
}

int lbc_replay_sample_launch(const double* cdf, int n, unsigned seed, unsigned long long step, int B, int* idx, hipStream_t s)
{
    LBC_REQUIRE(cdf && idx, "replay_sample: null argument");
    LBC_REQUIRE(n >= 1 && B >= 1, "replay_sample: n = %d, B = %d, both must be positive", n, B);
    LbcProfScope prof("replay_sample", 0.0, 4.0 * B, s);
    hipLaunchKernelGGL(sample_k, dim3((unsigned)lbc_cdiv(B, 256)), dim3(256), 0, s, cdf, n, seed, (unsigned)(step & 0xFFFFFFFFULL), (unsigned)(step >> 32), B, idx);
    return lbc_check_launch("replay_sample");
}

int lbc_replay_gather_launch(const unsigned char* src, long long row_bytes, const int* idx, int B, int reps, unsigned char* dst, hipStream_t s)
{
    LBC_REQUIRE(src && idx && dst, "replay_gather_u8: null argument");
    LBC_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0, "replay_gather_u8: row_bytes = %lld must be a positive multiple of 16 (rows move as 16-byte words)", row_bytes);
    LBC_REQUIRE(aligned16(src) && aligned16(dst), "replay_gather_u8: src and dst must be 16-byte aligned");
    LBC_REQUIRE(B >= 1 && reps >= 1, "replay_gather_u8: B = %d, reps = %d, both must be positive", B, reps);
    LbcProfScope prof("replay_gather_u8", 0.0, 2.0 * B * (double)reps * (double)row_bytes, s);
    row_copy_launch<true>(src, dst, idx, (long long)B * reps, reps, row_bytes, s);
    return lbc_check_launch("replay_gather_u8");
}

int lbc_replay_gather_indirect_launch(const unsigned char* src, long long row_bytes, const int* frame_of_slot, const int* idx, int B, int reps,
                                      unsigned char* dst, hipStream_t s)
{
    LBC_REQUIRE(src && frame_of_slot && idx && dst, "replay_gather_indirect_u8: null argument");
    LBC_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0, "replay_gather_indirect_u8: row_bytes = %lld must be a positive multiple of 16 (rows move as 16-byte words)",
                row_bytes);
    LBC_REQUIRE(aligned16(src) && aligned16(dst), "replay_gather_indirect_u8: src and dst must be 16-byte aligned");
    LBC_REQUIRE(B >= 1 && reps >= 1, "replay_gather_indirect_u8: B = %d, reps = %d, both must be positive", B, reps);
    LbcProfScope prof("replay_gather_indirect_u8", 0.0, 2.0 * B * (double)reps * (double)row_bytes, s);
    row_copy_launch<true, true>(src, dst, idx, (long long)B * reps, reps, row_bytes, s, frame_of_slot);
    return lbc_check_launch("replay_gather_indirect_u8");
}

size_t lbc_replay_admit_workspace_bytes(int limit, int m)
{
    if (limit < 1 || limit > kAdmitMax || m < 1 || m > kAdmitMax) return 0;
    return ((size_t)limit + 3 * (size_t)m) * 4;      // ukey [limit + m], rank [m], evslot [m]
}

int lbc_replay_admit_launch(float* weights, int* frame, int* cmd, float* speed, int* slot_of_frame, int F, int n, int limit, const float* cw,
                            const int* cframe, const int* ccmd, const float* cspeed, int m, void* workspace, size_t workspace_bytes, int* record,
                            hipStream_t s)
{
    LBC_REQUIRE(weights && frame && cmd && speed && slot_of_frame && cw && cframe && ccmd && cspeed && workspace && record, "replay_admit: null argument");
    LBC_REQUIRE(limit >= 1 && limit <= kAdmitMax, "replay_admit: limit = %d outside [1, %d] (one workgroup ranks the buffer)", limit, kAdmitMax);
    LBC_REQUIRE(m >= 1 && m <= kAdmitMax, "replay_admit: m = %d candidates outside [1, %d]", m, kAdmitMax);
    LBC_REQUIRE(n >= 0 && n <= limit, "replay_admit: n = %d occupied slots outside [0, limit = %d]", n, limit);
    LBC_REQUIRE(F >= 1, "replay_admit: F = %d frames, need at least one", F);
    LBC_REQUIRE(workspace_bytes >= lbc_replay_admit_workspace_bytes(limit, m), "replay_admit: workspace of %zu bytes, lbc_replay_admit_workspace(%d, %d) = %zu",
                workspace_bytes, limit, m, lbc_replay_admit_workspace_bytes(limit, m));
    unsigned* ukey = static_cast<unsigned*>(workspace);
    int* rank = reinterpret_cast<int*>(ukey + (size_t)limit + m);
    int* evslot = rank + m;
    LbcProfScope prof("replay_admit", 0.0, 4.0 * 40.0 * ((double)limit + m), s);
    hipLaunchKernelGGL(admit_k, dim3(1), dim3(kAdmitThreads), 0, s, weights, frame, cmd, speed, slot_of_frame, n, limit, cw, cframe, ccmd, cspeed, m, ukey, rank,
                       evslot, record);
    return lbc_check_launch("replay_admit");
}

int lbc_replay_scatter_launch(const unsigned char* src, long long row_bytes, const int* slot, int M, unsigned char* dst, hipStream_t s)
{
    LBC_REQUIRE(src && slot && dst, "replay_scatter_u8: null argument");
    LBC_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0, "replay_scatter_u8: row_bytes = %lld must be a positive multiple of 16 (rows move as 16-byte words)", row_bytes);
    LBC_REQUIRE(aligned16(src) && aligned16(dst), "replay_scatter_u8: src and dst must be 16-byte aligned");
    LBC_REQUIRE(M >= 1, "replay_scatter_u8: M = %d must be positive", M);
    LbcProfScope prof("replay_scatter_u8", 0.0, 2.0 * M * (double)row_bytes, s);
    row_copy_launch<false>(src, dst, slot, (long long)M, 1, row_bytes, s);
    return lbc_check_launch("replay_scatter_u8");
}

int lbc_replay_meta_launch(const float* speed, const int* cmd, const int* idx, int B, int reps, float* speed_out, float* onehot_out, hipStream_t s)
{
    LBC_REQUIRE(speed && cmd && idx && speed_out && onehot_out, "replay_meta: null argument");
    LBC_REQUIRE(B >= 1 && reps >= 1 && (long long)B * reps <= 0x7fffffffLL, "replay_meta: B = %d, reps = %d", B, reps);
    hipLaunchKernelGGL(meta_k, dim3((unsigned)lbc_cdiv((long long)B * reps, 256)), dim3(256), 0, s, speed, cmd, idx, B * reps, reps, speed_out, onehot_out);
    return lbc_check_launch("replay_meta");
}

int lbc_replay_writeback_launch(const float* w_batch, const int* idx, int B, int reps, int n, float* new_w, hipStream_t s)
{
    LBC_REQUIRE(w_batch && idx && new_w, "replay_writeback: null argument");
    LBC_REQUIRE(B >= 1 && B <= 1024, "replay_writeback: B = %d outside [1, 1024] (one workgroup resolves duplicate indices)", B);
    LBC_REQUIRE(reps >= 1 && n >= 1, "replay_writeback: reps = %d, n = %d, both must be positive", reps, n);
    hipLaunchKernelGGL(writeback_k, dim3(1), dim3((unsigned)(lbc_cdiv(B, 64) * 64)), 0, s, w_batch, idx, B, reps, n, new_w);
    return lbc_check_launch("replay_writeback");
}
