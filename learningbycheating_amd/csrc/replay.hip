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
//   meta       speed[idx] and one_hot(cmd[idx]) with the same fan-out.
//   writeback  new_w[idx[b]] = mean of the reps weights of source sample b; of equal indices the LAST b wins (numpy fancy assignment).
#include "lbc_common.hpp"
#include "lbc_hash.hpp"
#include "lbc_kernels.hpp"

namespace {

constexpr int kCdfThreads = 256;
constexpr int kCdfPerThread = 4;
constexpr int kCdfTile = kCdfThreads * kCdfPerThread;

// a weight the sampler can use: finite and >= 0 (NaN fails both comparisons)
__device__ __forceinline__ bool weight_ok(float w) { return w >= 0.f && w <= 3.402823466e38f; }

// inclusive scan of one value per thread over the workgroup (Hillis-Steele on two LDS planes); buf: 2 * blockDim.x doubles
__device__ __forceinline__ double block_scan_inclusive(double v, double* buf)
{
    const int t = (int)threadIdx.x, nt = (int)blockDim.x;
    int cur = 0;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < nt; d <<= 1) {
        const double x = buf[cur * nt + t] + (t >= d ? buf[cur * nt + t - d] : 0.0);
        buf[(cur ^ 1) * nt + t] = x;
        cur ^= 1;
        __syncthreads();
    }
    const double r = buf[cur * nt + t];
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
// y, y + gridDim.y, ...  GATHER: dst row r <- src row idx[r / reps]; else (scatter): dst row idx[r] <- src row r.
template <int U, bool GATHER>
__global__ __launch_bounds__(256) void row_copy_k(const uint4* __restrict__ src, uint4* __restrict__ dst, const int* __restrict__ idx, long long rows,
                                                  int reps, long long chunks_per_row)
{
    const long long c0 = (long long)blockIdx.x * (256 * U) + threadIdx.x;
    for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
        const long long other = (long long)idx[GATHER ? r / reps : r];
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

template <bool GATHER>
int row_copy_launch(const unsigned char* src, unsigned char* dst, const int* idx, long long rows, int reps, long long row_bytes, hipStream_t s)
{
    const long long cpr = row_bytes / 16;
    // 16 KB per workgroup once that still yields a thousand workgroups, 4 KB below (a batch of 4 frames: 180 instead of 48)
    const bool wide = rows * cpr >= 1024LL * 1024;
    const long long per = wide ? 1024 : 256;
    const dim3 grid((unsigned)((cpr + per - 1) / per), (unsigned)(rows < 65535 ? rows : 65535));
    if (wide)
        hipLaunchKernelGGL((row_copy_k<4, GATHER>), grid, dim3(256), 0, s, reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), idx, rows, reps, cpr);
    else
        hipLaunchKernelGGL((row_copy_k<1, GATHER>), grid, dim3(256), 0, s, reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), idx, rows, reps, cpr);
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
