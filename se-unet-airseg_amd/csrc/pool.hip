// Online hard mining on the device (reference train.py:78-138 save_data_online / save_data_online3, data.py:586-630
// OnlineHMData / OnlineHMData3), gfx950.
//
// The reference keeps the `limits` samples with the largest mining key as .npy files: every step copies the batch to the host,
// sorts the directory listing and writes / removes files.  Here the pool is a set of caller-owned HBM tensors
//   data (K, 2, V) f32   weight (K, 1, V) f32   label (K, 1, V) u8   [skel (K, 1, V) u8]   keys (K) f32   seq (K) i64
//   state (2) i64 = {count, next sequence number}
// and a step is two launches with no synchronise:
//   select   one block walks the batch in order like the loop of save_data_online and gives every sample a slot or -1;
//   scatter  grid (chunks, batch) copies the accepted samples into their slots, every stream with 16-byte accesses.
// gather writes the replay batches of train.py:479-481 back as f32.
#include "seunet_common.h"

namespace seunet {

// ---- select -----------------------------------------------------------------------------------------------------------------
// Order of the pool's entries: (key, seq), seq unique, so the minimum is unique and the wave-parallel search below gives
// the same slot however the entries are spread over the lanes.
struct PoolMin {
  float key;
  unsigned long long seq;
  int idx;
};
__device__ __forceinline__ bool pool_before(const PoolMin& a, const PoolMin& b) {
  return a.key < b.key || (a.key == b.key && a.seq < b.seq);
}

__global__ void __launch_bounds__(256)
pool_select_kernel(const float* __restrict__ new_keys, int batch, float* keys, long long* seq, long long* __restrict__ state, int capacity,
                   int* __restrict__ slots_out) {
  __shared__ int slots[SEUNET_POOL_MAX_BATCH];
  __shared__ PoolMin wave_min[4];
  long long count = state[0], next = state[1];       // every thread keeps its own copy; thread 0 stores them at the end
  if (count < 0) count = 0;
  if (count > capacity) count = capacity;
  for (int i = 0; i < batch; ++i) {
    const float key = new_keys[i];
    int slot = -1;
    if (isfinite(key)) {                              // a NaN or infinite key is never stored (the reference corrupts its list)
      if (count < capacity) {
        slot = (int)count;
      } else if (capacity > 0) {
        PoolMin m{INFINITY, ~0ull, -1};
        for (int j = threadIdx.x; j < capacity; j += 256) {
          const PoolMin c{keys[j], (unsigned long long)seq[j], j};
          if (pool_before(c, m)) m = c;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          const PoolMin o{shfl_xor_settled(m.key, off), shfl_xor_settled(m.seq, off), shfl_xor_settled(m.idx, off)};
          if (pool_before(o, m)) m = o;
        }
        if ((threadIdx.x & 63) == 0) wave_min[threadIdx.x >> 6] = m;
        __syncthreads();
        m = wave_min[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
          if (pool_before(wave_min[w], m)) m = wave_min[w];
        // bisect.bisect (train.py:94-95): only a key strictly below the minimum is dropped; one equal to it replaces it
        if (!(key < m.key)) slot = m.idx;
      }
    }
    if (slot >= 0) {
      if (threadIdx.x == 0) {
        keys[slot] = key;
        seq[slot] = next;
        for (int e = 0; e < i; ++e)                  // an earlier sample of this call that was given this slot loses it
          if (slots[e] == slot) slots[e] = -1;
      }
      if (count < capacity) ++count;
      ++next;
    }
    if (threadIdx.x == 0) slots[i] = slot;
    __syncthreads();                                  // keys / seq / slots / wave_min are settled before the next sample reads them
  }
  for (int i = threadIdx.x; i < batch; i += 256) slots_out[i] = slots[i];
  if (threadIdx.x == 0) {
    state[0] = count;
    state[1] = next;
  }
}

int launch_pool_select(const float* new_keys, int batch, float* keys, long long* seq, long long* state, int capacity, int* slots_out,
                       hipStream_t s) {
  SEUNET_CHECK(new_keys && state && slots_out, "pool_select: null argument");
  SEUNET_CHECK(batch >= 1 && batch <= SEUNET_POOL_MAX_BATCH, "pool_select: batch %d (1..%d)", batch, SEUNET_POOL_MAX_BATCH);
  SEUNET_CHECK(capacity >= 0 && capacity <= SEUNET_POOL_MAX_CAPACITY, "pool_select: capacity %d (0..%d)", capacity, SEUNET_POOL_MAX_CAPACITY);
  SEUNET_CHECK(capacity == 0 || (keys && seq), "pool_select: null keys / seq with capacity %d", capacity);
  pool_select_kernel<<<1, 256, 0, s>>>(new_keys, batch, keys, seq, state, capacity, slots_out);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// ---- scatter / gather -------------------------------------------------------------------------------------------------------
// A block moves POOL_CHUNK voxels of one sample: the f32 streams (two data channels, weight) as 16-byte loads and stores with
// consecutive lanes on consecutive float4, 4 per thread and stream; the 0/1 streams (label, skeleton) as four 16-byte loads of
// 16 consecutive voxels per thread against ONE 16-byte access of the packed bytes.  V % 16 == 0, so a thread's 16 voxels are
// inside the sample or outside it as a whole.
static constexpr int POOL_CHUNK = 4096;              // 256 threads x 16 voxels

__device__ __forceinline__ void copy_chunk(const float4* __restrict__ src, float4* __restrict__ dst, int n4) {
  const int i0 = threadIdx.x, i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a, d = a;
  if (i0 < n4) a = src[i0];                          // four loads in flight before the first store
  if (i1 < n4) b = src[i1];
  if (i2 < n4) c = src[i2];
  if (i3 < n4) d = src[i3];
  if (i0 < n4) dst[i0] = a;
  if (i1 < n4) dst[i1] = b;
  if (i2 < n4) dst[i2] = c;
  if (i3 < n4) dst[i3] = d;
}

__device__ __forceinline__ unsigned pack4(float4 v) {
  return (unsigned)(unsigned char)v.x | ((unsigned)(unsigned char)v.y << 8) | ((unsigned)(unsigned char)v.z << 16) |
         ((unsigned)(unsigned char)v.w << 24);
}
__device__ __forceinline__ float4 unpack4(unsigned u) {
  return make_float4((float)(u & 255u), (float)((u >> 8) & 255u), (float)((u >> 16) & 255u), (float)(u >> 24));
}
// 16 f32 -> 16 u8 (values 0.0 / 1.0; the conversion is (unsigned char)v), src / dst at this thread's 16 voxels
__device__ __forceinline__ void pack16(const float* __restrict__ src, unsigned char* __restrict__ dst) {
  const float4* s4 = reinterpret_cast<const float4*>(src);
  const float4 a = s4[0], b = s4[1], c = s4[2], d = s4[3];
  *reinterpret_cast<uint4*>(dst) = make_uint4(pack4(a), pack4(b), pack4(c), pack4(d));
}
__device__ __forceinline__ void unpack16(const unsigned char* __restrict__ src, float* __restrict__ dst) {
  const uint4 u = *reinterpret_cast<const uint4*>(src);
  float4* d4 = reinterpret_cast<float4*>(dst);
  d4[0] = unpack4(u.x); d4[1] = unpack4(u.y); d4[2] = unpack4(u.z); d4[3] = unpack4(u.w);
}

__global__ void __launch_bounds__(256)
pool_scatter_kernel(const int* __restrict__ slots, int capacity, long long V, const float* __restrict__ data, const float* __restrict__ label,
                    const float* __restrict__ weight, const float* __restrict__ skel, float* __restrict__ pool_data,
                    unsigned char* __restrict__ pool_label, float* __restrict__ pool_weight, unsigned char* __restrict__ pool_skel) {
  const int b = blockIdx.y;
  const long long slot = slots[b];
  if (slot < 0 || slot >= capacity) return;          // not stored (or not a slot of this pool: nothing is written)
  const long long v0 = (long long)blockIdx.x * POOL_CHUNK;
  const long long left = V - v0;
  const int n4 = (int)((left < POOL_CHUNK ? left : POOL_CHUNK) >> 2);
  copy_chunk(reinterpret_cast<const float4*>(data + (2ll * b) * V + v0), reinterpret_cast<float4*>(pool_data + (2 * slot) * V + v0), n4);
  copy_chunk(reinterpret_cast<const float4*>(data + (2ll * b + 1) * V + v0), reinterpret_cast<float4*>(pool_data + (2 * slot + 1) * V + v0), n4);
  copy_chunk(reinterpret_cast<const float4*>(weight + (long long)b * V + v0), reinterpret_cast<float4*>(pool_weight + slot * V + v0), n4);
  const long long v = v0 + threadIdx.x * 16;
  if (v < V) {
    pack16(label + (long long)b * V + v, pool_label + slot * V + v);
    if (skel) pack16(skel + (long long)b * V + v, pool_skel + slot * V + v);
  }
}

struct PoolSlots {
  int n;
  int slot[SEUNET_POOL_MAX_GATHER];
};

__global__ void __launch_bounds__(256)
pool_gather_kernel(PoolSlots sl, long long V, const float* __restrict__ pool_data, const unsigned char* __restrict__ pool_label,
                   const float* __restrict__ pool_weight, const unsigned char* __restrict__ pool_skel, float* __restrict__ data_out,
                   float* __restrict__ label_out, float* __restrict__ weight_out, float* __restrict__ skel_out) {
  const int b = blockIdx.y;
  const long long slot = sl.slot[b];
  const long long v0 = (long long)blockIdx.x * POOL_CHUNK;
  const long long left = V - v0;
  const int n4 = (int)((left < POOL_CHUNK ? left : POOL_CHUNK) >> 2);
  copy_chunk(reinterpret_cast<const float4*>(pool_data + (2 * slot) * V + v0), reinterpret_cast<float4*>(data_out + (2ll * b) * V + v0), n4);
  copy_chunk(reinterpret_cast<const float4*>(pool_data + (2 * slot + 1) * V + v0), reinterpret_cast<float4*>(data_out + (2ll * b + 1) * V + v0), n4);
  copy_chunk(reinterpret_cast<const float4*>(pool_weight + slot * V + v0), reinterpret_cast<float4*>(weight_out + (long long)b * V + v0), n4);
  const long long v = v0 + threadIdx.x * 16;
  if (v < V) {
    unpack16(pool_label + slot * V + v, label_out + (long long)b * V + v);
    if (skel_out) unpack16(pool_skel + slot * V + v, skel_out + (long long)b * V + v);
  }
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

static int pool_chunks(long long voxels, const char* what, int* chunks) {
  SEUNET_CHECK(voxels >= 16 && voxels % 16 == 0, "%s: %lld voxels per sample must be a positive multiple of 16", what, voxels);
  SEUNET_CHECK((voxels + POOL_CHUNK - 1) / POOL_CHUNK <= 0x7fffffffll, "%s: %lld voxels per sample is too many", what, voxels);
  *chunks = (int)((voxels + POOL_CHUNK - 1) / POOL_CHUNK);
  return 0;
}

int launch_pool_scatter(const int* slots_dev, int batch, int capacity, long long voxels, const float* data, const float* label,
                        const float* weight, const float* skel, float* pool_data, unsigned char* pool_label, float* pool_weight,
                        unsigned char* pool_skel, hipStream_t s) {
  SEUNET_CHECK(slots_dev && data && label && weight && pool_data && pool_label && pool_weight, "pool_scatter: null argument");
  SEUNET_CHECK((skel != nullptr) == (pool_skel != nullptr), "pool_scatter: skel and pool_skel go together");
  SEUNET_CHECK(batch >= 1 && batch <= SEUNET_POOL_MAX_BATCH, "pool_scatter: batch %d (1..%d)", batch, SEUNET_POOL_MAX_BATCH);
  SEUNET_CHECK(capacity >= 1 && capacity <= SEUNET_POOL_MAX_CAPACITY, "pool_scatter: capacity %d (1..%d)", capacity, SEUNET_POOL_MAX_CAPACITY);
  SEUNET_CHECK(aligned16(data) && aligned16(label) && aligned16(weight) && aligned16(skel) && aligned16(pool_data) &&
               aligned16(pool_label) && aligned16(pool_weight) && aligned16(pool_skel), "pool_scatter: every tensor must be 16-byte aligned");
  int chunks = 0;
  if (pool_chunks(voxels, "pool_scatter", &chunks)) return 1;
  pool_scatter_kernel<<<dim3(chunks, batch), 256, 0, s>>>(slots_dev, capacity, voxels, data, label, weight, skel, pool_data, pool_label,
                                                           pool_weight, pool_skel);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_pool_gather(const int* slots_host, int n, int capacity, long long voxels, const float* pool_data,
                       const unsigned char* pool_label, const float* pool_weight, const unsigned char* pool_skel, float* data_out,
                       float* label_out, float* weight_out, float* skel_out, hipStream_t s) {
  SEUNET_CHECK(slots_host && pool_data && pool_label && pool_weight && data_out && label_out && weight_out, "pool_gather: null argument");
  SEUNET_CHECK(!skel_out || pool_skel, "pool_gather: skeleton output from a pool without skeletons");
  SEUNET_CHECK(n >= 1 && n <= SEUNET_POOL_MAX_GATHER, "pool_gather: %d samples per call (1..%d)", n, SEUNET_POOL_MAX_GATHER);
  SEUNET_CHECK(capacity >= 1 && capacity <= SEUNET_POOL_MAX_CAPACITY, "pool_gather: capacity %d (1..%d)", capacity, SEUNET_POOL_MAX_CAPACITY);
  SEUNET_CHECK(aligned16(pool_data) && aligned16(pool_label) && aligned16(pool_weight) && aligned16(pool_skel) && aligned16(data_out) &&
               aligned16(label_out) && aligned16(weight_out) && aligned16(skel_out), "pool_gather: every tensor must be 16-byte aligned");
  PoolSlots sl;
  sl.n = n;
  for (int k = 0; k < n; ++k) {
    SEUNET_CHECK(slots_host[k] >= 0 && slots_host[k] < capacity, "pool_gather: slot %d of sample %d is outside the pool of %d", slots_host[k], k, capacity);
    sl.slot[k] = slots_host[k];
  }
  int chunks = 0;
  if (pool_chunks(voxels, "pool_gather", &chunks)) return 1;
  pool_gather_kernel<<<dim3(chunks, n), 256, 0, s>>>(sl, voxels, pool_data, pool_label, pool_weight, pool_skel, data_out, label_out,
                                                      weight_out, skel_out);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
