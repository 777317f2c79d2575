// 3-D binary morphology with the 6-neighbour cross on the device: the dilation and closing of the reference's own airway parser
// (DESIGN.md section 3g).
//
// Reference (CPU, skimage behind it):
//   ours_skel_parse.py:577-578   LABEL_TRANS = binary_closing(binary_fill_holes(binary_dilation(label))): skimage.morphology with
//                                its default footprint, the cross of the 6 face neighbours.  Closing = dilation, then erosion.
//                                Outside the volume counts as 0 for a dilation and as 1 for the erosion of a closing (the reading
//                                of skimage 0.21-0.24 = scipy's binary_erosion(border_value=True); not checked against skimage).
// Volumes are bit-packed along axis 2 (bit j of word w of a row = voxel 64 w + j, as in skeleton.hip and dti.hip).  A word's
// result is its own two shifts with the carry bits of the neighbouring words, combined with the same word of the four
// neighbouring rows: OR for a dilation, AND for an erosion.  A neighbour outside the volume and the tail bits of a row's last
// word read as the operation's border value; results are masked to the valid bits, so a packed volume always has zero tails.
// CLOSE runs the DILATE and the ERODE_BORDER1 step back to back on the packed words: it IS one after the other, bit for bit.
// Integer / bit work: results are bit-identical to scipy's (tests/test_airway_parse_gpu.py).
#include "volume.h"

namespace seunet {

// bytes -> bits: one wave per word, lane j reads voxel 64 w + j of the row (coalesced), the ballot is the word
__global__ void __launch_bounds__(256)
morph_pack_kernel(const unsigned char* __restrict__ vol, long long rows, int n2, int nw, u64* __restrict__ bits) {
  const long long word = blockIdx.x * 4ll + (threadIdx.x >> 6);      // wave-uniform
  if (word >= rows * nw) return;
  const int lane = threadIdx.x & 63;
  const long long row = word / nw;
  const int k = (int)(word % nw) * 64 + lane;
  const bool on = k < n2 && vol[row * n2 + k] != 0;
  const u64 m = __ballot(on);
  if (lane == 0) bits[word] = m;
}

// one step on packed words, one thread per word.  ERODE: false = dilation (outside = 0); true = erosion with outside = `border`.
template <bool ERODE>
__global__ void __launch_bounds__(256)
morph_step_kernel(const u64* __restrict__ in, int n0, int n1, int n2, int nw, bool border, u64* __restrict__ out) {
  const long long rows = (long long)n0 * n1;
  const long long idx = blockIdx.x * 256ll + threadIdx.x;
  if (idx >= rows * nw) return;
  const long long row = idx / nw;
  const int m = (int)(idx % nw);
  const int i1 = (int)(row % n1), i0 = (int)(row / n1);
  const u64 valid = (m + 1 < nw || (n2 & 63) == 0) ? ~0ull : ((1ull << (n2 & 63)) - 1ull);
  const u64 outside = (ERODE && border) ? ~0ull : 0ull;
  const u64 x = in[idx] | (outside & ~valid);                           // the tail reads as the border value
  const u64 lo = m > 0 ? in[idx - 1] >> 63 : outside & 1ull;            // voxel 64 m - 1
  const u64 hi = m + 1 < nw ? in[idx + 1] << 63 : outside << 63;        // voxel 64 m + 64 (bit 0 of the next word is always valid)
  const long long plane = (long long)n1 * nw;
  const u64 r0 = i1 > 0 ? in[idx - nw] : outside;
  const u64 r1 = i1 + 1 < n1 ? in[idx + nw] : outside;
  const u64 p0 = i0 > 0 ? in[idx - plane] : outside;
  const u64 p1 = i0 + 1 < n0 ? in[idx + plane] : outside;
  const u64 down = (x << 1) | lo, upw = (x >> 1) | hi;
  const u64 r = ERODE ? (x & down & upw & r0 & r1 & p0 & p1) : (x | down | upw | r0 | r1 | p0 | p1);
  out[idx] = r & valid;
}

__global__ void __launch_bounds__(256)
morph_unpack_kernel(const u64* __restrict__ bits, long long rows, int n2, int nw, unsigned char* __restrict__ out) {
  const long long idx = blockIdx.x * 256ll + threadIdx.x;
  if (idx >= rows * n2) return;
  const long long row = idx / n2;
  const int k = (int)(idx % n2);
  out[idx] = (unsigned char)((bits[row * nw + (k >> 6)] >> (k & 63)) & 1ull);
}

size_t binary_morph_workspace_bytes(int n0, int n1, int n2) { return measured(morph_ws, n0, n1, n2); }

int launch_binary_morph(const unsigned char* vol, int n0, int n1, int n2, int op, unsigned char* out, void* workspace, size_t ws_bytes,
                        hipStream_t s) {
  SEUNET_CHECK(vol && out && workspace, "binary_morph: null argument");
  SEUNET_CHECK(vol != out, "binary_morph: out may not alias volume");
  SEUNET_CHECK(op >= 0 && op <= 3, "binary_morph: op %d (0 = dilate, 1 = erode with outside 0, 2 = erode with outside 1, 3 = close)", op);
  if (volume_check("binary_morph", n0, n1, n2, 0)) return 1;
  WsCarver carve(workspace);
  const MorphWs w = morph_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "binary_morph: workspace too small");
  const int nw = (n2 + 63) / 64;
  const long long rows = (long long)n0 * n1, words = rows * nw;
  morph_pack_kernel<<<(unsigned)((words + 3) / 4), 256, 0, s>>>(vol, rows, n2, nw, w.a);
  const u64* result = w.b;
  switch (op) {
    case 0: morph_step_kernel<false><<<blocks_256(words), 256, 0, s>>>(w.a, n0, n1, n2, nw, false, w.b); break;
    case 1: morph_step_kernel<true><<<blocks_256(words), 256, 0, s>>>(w.a, n0, n1, n2, nw, false, w.b); break;
    case 2: morph_step_kernel<true><<<blocks_256(words), 256, 0, s>>>(w.a, n0, n1, n2, nw, true, w.b); break;
    default:
      morph_step_kernel<false><<<blocks_256(words), 256, 0, s>>>(w.a, n0, n1, n2, nw, false, w.b);
      morph_step_kernel<true><<<blocks_256(words), 256, 0, s>>>(w.b, n0, n1, n2, nw, true, w.a);
      result = w.a;
  }
  morph_unpack_kernel<<<blocks_256(rows * n2), 256, 0, s>>>(result, rows, n2, nw, out);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
