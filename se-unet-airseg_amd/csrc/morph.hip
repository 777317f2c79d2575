// 3-D binary morphology with the 6-neighbour cross on the device: the dilation and closing of the reference's own airway parser
// (DESIGN.md section 3g).
//
// Reference (CPU, skimage behind it):
//   ours_skel_parse.py:577-578   LABEL_TRANS = binary_closing(binary_fill_holes(binary_dilation(label))): skimage.morphology with
//                                its default footprint, the cross of the 6 face neighbours.  Closing = dilation, then erosion.
//                                Outside the volume counts as 0 for a dilation and as 1 for the erosion of a closing (the reading
//                                of skimage 0.21-0.24 = scipy's binary_erosion(border_value=True); not checked against skimage).
// Volumes are bit-packed along axis 2 (bitvol.h).  A word's result is the OR (dilation) or the AND (erosion)
// of load_cross6: its own two shifts with the carry bits of the neighbouring words and the same word of the four neighbouring
// rows.  A neighbour outside the volume and the tail bits of a row's last word read as the operation's border value; results are
// masked to the valid bits, so a packed volume always has zero tails.
// CLOSE runs the DILATE and the ERODE_BORDER1 step back to back on the packed words: it IS one after the other, bit for bit.
// Integer / bit work: results are bit-identical to scipy's (tests/test_airway_parse_gpu.py).
#include "volume.h"

namespace seunet {

// one step on packed words, one thread per word.  ERODE: false = dilation (outside = 0); true = erosion with outside = `border`.
template <bool ERODE>
__global__ void __launch_bounds__(256) morph_step_kernel(const u64* __restrict__ in, BitGeom g, bool border, u64* __restrict__ out) {
  const long long idx = blockIdx.x * 256ll + threadIdx.x;
  if (idx >= g.words) return;
  const Cross6 c = load_cross6(in, g, idx, (ERODE && border) ? ~0ull : 0ull);
  out[idx] = (ERODE ? and6(c) : or6(c)) & c.valid;
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
  const BitGeom g = bit_geom(n0, n1, n2);
  const unsigned blocks = blocks_256(g.words);
  pack_bits(vol, nullptr, g, w.a, nullptr, s);
  const u64* result = w.b;
  switch (op) {
    case 0: morph_step_kernel<false><<<blocks, 256, 0, s>>>(w.a, g, false, w.b); break;
    case 1: morph_step_kernel<true><<<blocks, 256, 0, s>>>(w.a, g, false, w.b); break;
    case 2: morph_step_kernel<true><<<blocks, 256, 0, s>>>(w.a, g, true, w.b); break;
    default:
      morph_step_kernel<false><<<blocks, 256, 0, s>>>(w.a, g, false, w.b);
      morph_step_kernel<true><<<blocks, 256, 0, s>>>(w.b, g, true, w.a);
      result = w.a;
  }
  unpack_bits(result, g, out, s);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
