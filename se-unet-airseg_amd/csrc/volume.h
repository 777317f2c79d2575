// Shared layer of the volume operations (components.hip, lung.hip, edt.hip, edt_sampling.hip, parse.hip, skeleton.hip, dti.hip,
// morph.hip, mesh.hip, mesh_label.hip, morphometry.hip, cldice.hip, surface.hip, betti.hip, cross_section.hip): their launcher prototypes, ONE
// workspace layout per operation, the extent check and the voxel / wave helpers their kernels share.  The bit-packed
// representation seven of them work on -- geometry, packing, neighbour words, the scan, wave counts -- is bitvol.h / bitvol.hip.
//
// Workspace contract: every operation has a layout struct filled by one function that walks a WsCarver.  Over a null base
// the walk measures (`X_workspace_bytes`), over the caller's workspace it carves (the launcher); no launcher computes an
// offset of its own, so a buffer cannot be added to one side only.  seunet_debug_volume_layout (abi.cpp) reports the same walk
// to tests/test_volume_layout_host.py, which pins the byte counts.
#pragma once
#include "seunet_common.h"
#include "bitvol.h"
#include <algorithm>

namespace seunet {

// workgroups of a one-thread-per-item pass of 256-thread blocks (grid_for clamps to 4096 workgroups for grid-stride passes)
static inline unsigned blocks_256(long long n) { return (unsigned)((n + 255) / 256); }

// Bump carver over a device workspace, the sibling of Plan::take in net.cpp (which hands out offsets of a workspace it never sees,
// and logs a name with each: seunet_debug_net_layout).  A null base measures: take() returns null and
// only the offset advances.  `log` (the layout report only; null in queries and launchers) receives the offset of every take.
struct WsCarver {
  unsigned char* base;
  size_t off = 0;
  size_t* log = nullptr;
  int log_cap = 0, taken = 0;
  explicit WsCarver(void* workspace) : base(reinterpret_cast<unsigned char*>(workspace)) {}
  template <typename T> T* take(size_t count, size_t align = 256) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    if (taken < log_cap) log[taken] = off;
    ++taken;
    off += align_up(count * sizeof(T), align);
    return p;
  }
  size_t bytes() const { return off; }
};
// what a layout function carves in all: the body of every X_workspace_bytes
template <typename Layout> size_t measured(Layout layout, int n0, int n1, int n2) {
  WsCarver c(nullptr);
  layout(c, n0, n1, n2);
  return c.bytes();
}

// Extent checks of the launchers.  max_extent 0: no per-axis limit (32767 where features are int16, edt.hip).  label_range:
// the wording of components.hip / lung.hip, whose labels are the 32-bit linear indices.
static inline int volume_check(const char* what, int n0, int n1, int n2, int max_extent, bool label_range = false) {
  SEUNET_CHECK(n0 >= 1 && n1 >= 1 && n2 >= 1, "%s: bad extents (%d, %d, %d)", what, n0, n1, n2);
  SEUNET_CHECK(max_extent == 0 || (n0 <= max_extent && n1 <= max_extent && n2 <= max_extent),
               "%s: extents (%d, %d, %d): at most %d per axis", what, n0, n1, n2, max_extent);
  const long long n = (long long)n0 * n1 * n2;
  SEUNET_CHECK(n < (1ll << 31),
               label_range ? "%s: %lld voxels exceed the 32-bit label range" : "%s: %lld voxels: fewer than 2^31 supported", what, n);
  return 0;
}
constexpr int kEdtMaxExtent = 32767;      // features are int16 between the EDT passes

// ---- connected components / metrics (components.hip) --------------------------------------------------------------------
// Union-find on labels = minimum linear index (every element points to a smaller index of its set, roots to themselves; a union
// is an atomicMin on the larger root).  Parents only decrease, so a stale read is still an ancestor and cc_find terminates.
// Shared with the per-slice labelling of lung.hip.
__device__ __forceinline__ int cc_find(const int* L, int i) {
  int p = L[i];
  while (p != i) { i = p; p = L[i]; }      // strictly decreasing chain: terminates even on stale reads
  return i;
}

__device__ __forceinline__ void cc_union(int* L, int a, int b) {
  bool done;
  do {
    a = cc_find(L, a);
    b = cc_find(L, b);
    if (a < b) { const int old = atomicMin(&L[b], a); done = old == b; b = old; }
    else if (b < a) { const int old = atomicMin(&L[a], b); done = old == a; a = old; }
    else done = true;
  } while (!done);
}

struct CcSel {            // device-side scalars of one call
  u64 best, second;       // (voxel count << 32) | root index ; 0 = none
  int touches;            // largest component has a voxel in one of the three test slices
  int chosen;             // root index of the selected component, -1 = none
  int status;             // 0 ok, 1 no component at all, 2 second component needed but absent
  int pad;
};

struct CcWs {
  int* labels;
  unsigned int* counts;   // voxel counts per root, then the border flags of the hole filling
  CcSel* sel;
};
static inline CcWs cc_ws(WsCarver& c, int H, int W, int Z) {
  const size_t n = (size_t)H * W * Z;
  return CcWs{c.take<int>(n), c.take<unsigned int>(n), c.take<CcSel>(1)};   // (a braced list is evaluated left to right)
}

size_t cc_workspace_bytes(int H, int W, int Z);
void cc_label26(const unsigned char* vol, int H, int W, int Z, int* L, hipStream_t s);   // component labels (minimum index), -1 off
int launch_largest_component(const unsigned char* vol, int H, int W, int Z, int rule, unsigned char* out, int* status_dev,
                             void* workspace, size_t ws_bytes, hipStream_t s);
// scipy.ndimage.binary_fill_holes: out = (vol != 0) plus the 6-connected background that does not reach the border; workspace: cc_ws
int launch_fill_holes(const unsigned char* vol, int H, int W, int Z, unsigned char* out, void* workspace, size_t ws_bytes, hipStream_t s);
void launch_cc_compress(int* L, long long n, hipStream_t s);                          // L[i] = root of i
void launch_cc_count(const int* L, long long n, unsigned int* cnt, hipStream_t s);   // cnt[root] += voxels (cnt zeroed by the caller)
size_t metric_out_bytes(int nbins);
int launch_metric_sums(const unsigned char* pred, const unsigned char* label, const unsigned char* skel, const int* parsing, long long n,
                       int nbins, void* out, size_t out_bytes, hipStream_t s);

// ---- stage-2/3 preparation (edt.hip): exact EDT / feature transform, candidate bit masks, LIB weight, break weight ---------
size_t edt_workspace_bytes(int n0, int n1, int n2);
struct EdtWs {
  short *f0, *fa, *fb;    // features along axis 0 after pass 0; along axes 0 / 1 after pass 1
  short* spos;            // the stack of each line: positions
  int* sr;                //                         off-line offsets
};
static inline EdtWs edt_ws(WsCarver& c, int n0, int n1, int n2) {
  const size_t n = (size_t)n0 * n1 * n2;
  return EdtWs{c.take<short>(n), c.take<short>(n), c.take<short>(n), c.take<short>(n), c.take<int>(n)};
}

struct LibWeightWs { unsigned char *c2, *c12; };   // 7-tap counts along axis 2, then along axes 1 and 2
static inline LibWeightWs lib_weight_ws(WsCarver& c, int n0, int n1, int n2) {
  const size_t n = (size_t)n0 * n1 * n2;
  return LibWeightWs{c.take<unsigned char>(n), c.take<unsigned char>(n)};
}

struct BreakWeightWs {
  EdtWs edt;              // one whole EDT workspace (run_edt lays it out again): edt_bytes from edt.f0 on
  size_t edt_bytes;
  int *lin, *labels;      // feature (linear index) of every voxel; component labels of fn_skel
  unsigned char *fn, *flag, *brs, *brl, *shell;
  u64* maxf;
};
static inline BreakWeightWs break_weight_ws(WsCarver& c, int n0, int n1, int n2) {
  const size_t n = (size_t)n0 * n1 * n2;
  BreakWeightWs w;
  w.edt_bytes = edt_workspace_bytes(n0, n1, n2);
  WsCarver edt(c.take<unsigned char>(w.edt_bytes));
  w.edt = edt_ws(edt, n0, n1, n2);
  w.lin = c.take<int>(n);
  w.labels = c.take<int>(n);
  w.fn = c.take<unsigned char>(n);
  w.flag = c.take<unsigned char>(n);
  w.brs = c.take<unsigned char>(n);
  w.brl = c.take<unsigned char>(n);
  w.shell = c.take<unsigned char>(n);
  w.maxf = c.take<u64>(1);
  return w;
}

int launch_edt(const unsigned char* vol, int n0, int n1, int n2, int* sqdist, double* dist, int* indices, int* status_dev,
               void* workspace, size_t ws_bytes, hipStream_t s);
struct EdtOut {            // what the last pass of the feature transform writes (each part optional)
  int* sqdist;
  double* dist;
  int* indices;            // (3, n0, n1, n2)
  int* lin;                // linear index of the feature (internal users)
  const int* gather_src;   // gather_out[v] = gather_mask[v] != 0 ? gather_src[feature of v] : 0 (all three or none)
  const unsigned char* gather_mask;
  int* gather_out;
};
// invert = false: sites are the zero voxels (distance_transform_edt(vol)); true: the non-zero ones (EDT of 1 - vol)
int run_edt(const unsigned char* vol, bool invert, int n0, int n1, int n2, EdtOut o, int* status_dev, void* workspace, size_t ws_bytes,
            hipStream_t s);
// pass 0 alone: f0 = coordinate along axis 0 of the nearest site of each column (-1: none); status_dev (optional) = 1 without a site
int run_edt_pass0(const unsigned char* vol, bool invert, int n0, int n1, int n2, short* f0, int* status_dev, hipStream_t s);

// ---- EDT with voxel spacing (edt_sampling.hip): pass 0 of edt.hip, then passes 1 and 2 in float64 ---------------------------
struct EdtSamplingWs {
  short *f0, *fa, *fb;    // as EdtWs
  short* spos;            // the stack of each line: positions only (the off-line terms are recomputed from the features)
};
static inline EdtSamplingWs edt_sampling_ws(WsCarver& c, int n0, int n1, int n2) {
  const size_t n = (size_t)n0 * n1 * n2;
  return EdtSamplingWs{c.take<short>(n), c.take<short>(n), c.take<short>(n), c.take<short>(n)};
}
struct EdtSamplingOut {    // what the last pass writes (each part optional)
  double* dist;
  int* indices;            // (3, n0, n1, n2)
  int* lin;                // linear index of the feature
};
size_t edt_sampling_workspace_bytes(int n0, int n1, int n2);
int launch_edt_sampling(const unsigned char* vol, int n0, int n1, int n2, double s0, double s1, double s2, EdtSamplingOut o,
                        int* status_dev, void* workspace, size_t ws_bytes, hipStream_t s);

int launch_mask_bits(const unsigned char* mask, long long n, unsigned long long* bits, hipStream_t s);
int launch_hm_candidates(const unsigned char* label, const unsigned char* skel, const unsigned char* pred, int n0, int n1, int n2,
                         unsigned long long* skel_bits, unsigned long long* small_bits, hipStream_t s);
size_t lib_weight_workspace_bytes(int n0, int n1, int n2);
int launch_lib_weight(const unsigned char* label, int n0, int n1, int n2, const float* table, void* out, void* workspace,
                      size_t ws_bytes, hipStream_t s);
size_t break_weight_workspace_bytes(int n0, int n1, int n2);
int launch_break_weight(const unsigned char* label, const unsigned char* pred, const unsigned char* skel, int n0, int n1, int n2,
                        void* w_br, unsigned char* br_skel, int* status_dev, void* workspace, size_t ws_bytes, hipStream_t s);

// ---- 3-D thinning (skeleton.hip); workspace bytes are 0 for extents the bit layout cannot address -------------------------
size_t skeleton_workspace_bytes(int n0, int n1, int n2);
bool skeleton_ws(WsCarver& c, int n0, int n1, int n2);     // the walk of SkelLayout alone (layout report); false: rejected extents
int launch_skeletonize(const unsigned char* vol, int n0, int n1, int n2, unsigned char* out, int* passes_dev, void* workspace,
                       size_t ws_bytes, hipStream_t s);

// ---- airway tree parsing (parse.hip): skeleton branches, nearest-branch assignment, label statistics, relabelling ---------
struct BranchesWs {
  int* labels;
  unsigned int* counts;          // voxels per root, then the root's number
  unsigned char* keep;           // skeleton voxels that are no branch points
  unsigned int* block_roots;     // surviving roots per block of 256 voxels, then their prefix sums
};
static inline BranchesWs branches_ws(WsCarver& c, int n0, int n1, int n2) {
  const size_t n = (size_t)n0 * n1 * n2;
  return BranchesWs{c.take<int>(n), c.take<unsigned int>(n), c.take<unsigned char>(n), c.take<unsigned int>((n + 255) / 256)};
}

size_t skeleton_branches_workspace_bytes(int n0, int n1, int n2);
int launch_skeleton_branches(const unsigned char* skel, int n0, int n1, int n2, int min_voxels, int* cd, unsigned char* skeleton_parse,
                             int* num_dev, void* workspace, size_t ws_bytes, hipStream_t s);
size_t parse_assign_workspace_bytes(int n0, int n1, int n2);
int launch_parse_assign(const unsigned char* skeleton_parse, const int* cd, const unsigned char* label, int n0, int n1, int n2,
                        int* parsing, int* status_dev, void* workspace, size_t ws_bytes, hipStream_t s);
int label_stats_max_num();
int launch_label_stats(const int* parsing, int n0, int n1, int n2, int num, unsigned int* counts, unsigned long long* adjacency_bits,
                       int* status_dev, hipStream_t s);
int launch_relabel(const int* parsing, long long n, const int* lut, int nlut, int* out, hipStream_t s);
// the reference's own parser: centroid sums of one axis-2 slice, and cd / skeleton_parse from a voxel list
int launch_slice_moments(const unsigned char* mask, int n0, int n1, int n2, int k, unsigned long long* out_dev, hipStream_t s);
int launch_scatter_labels(const long long* lin_index, const int* value, long long m, long long n, int* cd, unsigned char* skeleton_parse,
                          int* status_dev, hipStream_t s);

// ---- binary morphology with the 6-neighbour cross (morph.hip) ---------------------------------------------------------------
struct MorphWs { u64 *a, *b; };   // the packed volume and one step's result; rows of ceil(n2 / 64) words
static inline MorphWs morph_ws(WsCarver& c, int n0, int n1, int n2) {
  const size_t nwords = words(n0, n1, n2);
  return MorphWs{c.take<u64>(nwords), c.take<u64>(nwords)};
}
size_t binary_morph_workspace_bytes(int n0, int n1, int n2);
int launch_binary_morph(const unsigned char* vol, int n0, int n1, int n2, int op, unsigned char* out, void* workspace, size_t ws_bytes,
                        hipStream_t s);

// ---- CT preprocessing (lung.hip): value counts, shift + clamp, per-slice lung field, mask combination, bounding box, crop --
struct GetLWs {
  int* labels;
  unsigned int* counts;          // pixels per root, then the border flags
  u64 *best, *top1, *top2;       // per-slice keys, back to back: one memset of key_bytes from `best` clears the three
  size_t key_bytes;
};
static inline GetLWs get_l_ws(WsCarver& c, int H, int W, int Z) {
  const size_t n = (size_t)H * W * Z;
  GetLWs w;
  w.labels = c.take<int>(n);
  w.counts = c.take<unsigned int>(n);
  const size_t keys_at = c.bytes();
  w.best = c.take<u64>((size_t)Z);
  w.top1 = c.take<u64>((size_t)Z);
  w.top2 = c.take<u64>((size_t)Z);
  w.key_bytes = c.bytes() - keys_at;
  return w;
}

int launch_value_counts(const short* ct, long long n, int shift, unsigned int* counts, hipStream_t s);
int launch_shift_clamp(const short* ct, long long n, int shift, int clamp, int clamp_le, int clamp_to, short* out, hipStream_t s);
size_t get_l_workspace_bytes(int H, int W, int Z);
int launch_get_l(const short* ct, int H, int W, int Z, double T, int min_area, unsigned char* out, void* workspace, size_t ws_bytes,
                 hipStream_t s);
int launch_mask_combine(const unsigned char* a, const unsigned char* b, long long n, int op, unsigned char* out, hipStream_t s);
int launch_mask_box(const unsigned char* mask, int H, int W, int Z, int* box, hipStream_t s);
int launch_crop3d(const void* src, int elem_bytes, int H, int W, int Z, const int* box, void* dst, hipStream_t s);

// ---- double threshold (dti.hip) -------------------------------------------------------------------------------------------
struct DtiWs { u64 *g, *weak; };   // strong mask (swept in place into the result), weak mask; rows of ceil(z / 64) words
static inline DtiWs dti_ws(WsCarver& c, int h, int w, int z) {
  const size_t nwords = words(h, w, z);
  return DtiWs{c.take<u64>(nwords, 8), c.take<u64>(nwords, 8)};   // the two halves have never been padded: word alignment only
}
size_t dti_workspace_bytes(int h, int w, int z);
int launch_dti(const double* pred, int h, int w, int z, double h_thresh, double l_thresh, int pred_dtype, unsigned char* out,
               void* workspace, size_t ws_bytes, hipStream_t s);

// ---- surface meshing (mesh.hip): extraction, vertex adjacency, smoothing, affine step, STL records ---------------------------
struct MeshRec { u64 nverts, nfaces; };   // the totals the host reads once
struct MeshWs {
  MeshRec* rec;
  u64* bits;                      // the packed volume; rows of ceil(n2 / 64) words, no padding
  u64 *a0, *a1, *a2;              // per word: the voxels that own a vertex along axis 0, 1, 2
  unsigned *vcnt, *fcnt;          // per word: vertices and triangles, then their exclusive scan inside a block of 1024 words
  unsigned *vblk, *fblk;          // per block: its total, then the exclusive scan of the totals
};
static inline MeshWs mesh_ws(WsCarver& c, int n0, int n1, int n2) {
  const size_t nwords = words(n0, n1, n2), blocks = (nwords + kScanBlock - 1) / kScanBlock;
  return MeshWs{c.take<MeshRec>(1), c.take<u64>(nwords), c.take<u64>(nwords), c.take<u64>(nwords), c.take<u64>(nwords),
                c.take<unsigned>(nwords), c.take<unsigned>(nwords), c.take<unsigned>(blocks), c.take<unsigned>(blocks)};
}
struct MeshAdjWs {
  u64* total;                     // the scan's grand total (two slots)
  unsigned* deg;                  // V + 1: list lengths, then the fill cursors, then the lengths without repeats
  unsigned* rawptr;               // V + 1: start of every vertex's list in raw
  unsigned* raw;                  // 6 F: (neighbour << 1) | arrives, later the sorted neighbours at the front of each list
  unsigned* blk;                  // block totals of the scans
};
static inline MeshAdjWs mesh_adj_ws(WsCarver& c, long long nverts, long long nfaces) {
  const size_t v1 = (size_t)nverts + 1;
  return MeshAdjWs{c.take<u64>(2), c.take<unsigned>(v1), c.take<unsigned>(v1), c.take<unsigned>((size_t)nfaces * 6),
                   c.take<unsigned>((v1 + 1023) / 1024)};
}
size_t mesh_workspace_bytes(int n0, int n1, int n2);
size_t mesh_adjacency_workspace_bytes(long long nverts, long long nfaces);
// count: pack, count, scan; synchronises once to return the totals.  emit: verts (V, 3) and faces (F, 3) from the same workspace.
int launch_mesh_count(const unsigned char* vol, int n0, int n1, int n2, long long* nverts, long long* nfaces, void* workspace,
                      size_t ws_bytes, hipStream_t s);
int launch_mesh_emit(int n0, int n1, int n2, double level, long long nverts, long long nfaces, float* verts, int* faces,
                     const void* workspace, size_t ws_bytes, hipStream_t s);
int launch_mesh_coord_sums(const unsigned char* mask, int n0, int n1, int n2, long long* sums_dev, hipStream_t s);
int launch_mesh_adjacency(const int* faces, long long nfaces, long long nverts, int* indptr, int* indices, long long capacity,
                          unsigned char* boundary, int* status_dev, void* workspace, size_t ws_bytes, hipStream_t s);
int launch_mesh_smooth(const float* verts, long long nverts, const int* indptr, const int* indices, const unsigned char* boundary,
                       int n_iter, float relaxation, float* out, float* tmp, hipStream_t s);
int launch_mesh_affine(const float* verts, long long nverts, const float* centre, const float* scale, float* out, hipStream_t s);
int launch_mesh_stl_records(const float* verts, long long nverts, const int* faces, long long nfaces, const float* centre,
                            const float* scale, unsigned char* records, int* status_dev, hipStream_t s);

// ---- labelled surface meshing (mesh_label.hip): every label's mesh of an int32 label volume in one extraction ----------------
constexpr int kMeshLabelMax = 65535;      // labels are 16-bit sort keys: two radix digits
struct MeshLabelRec { u64 nverts, nfaces; int max_label, status; };   // what the host reads once; status: 1 negative, 2 too large
struct MeshLabelWs {
  MeshLabelRec* rec;
  u64 *vb0, *vb1, *vb2;           // per word: bit planes of the vertex count (0 .. 6) of each of its voxels
  unsigned *vcnt, *fcnt;          // per word: vertex and triangle items, then their exclusive scan inside a block of 1024 words
  unsigned char* active;          // per word: 1 where the word has an item at all; the emit passes leave the others at once
  unsigned *vblk, *fblk;          // per block: its total, then the exclusive scan of the totals
  unsigned *vhist, *fhist;        // kMeshLabelMax + 1 each: items per label, then their exclusive scan inside a block
  unsigned *hvblk, *hfblk;        // the block totals of the two label scans
  u64* htotal;                    // their grand totals (two slots)
};
static inline MeshLabelWs mesh_label_ws(WsCarver& c, int n0, int n1, int n2) {
  const size_t nwords = words(n0, n1, n2), blocks = (nwords + kScanBlock - 1) / kScanBlock;
  const size_t labels = kMeshLabelMax + 1, label_blocks = labels / kScanBlock;
  return MeshLabelWs{c.take<MeshLabelRec>(1), c.take<u64>(nwords), c.take<u64>(nwords), c.take<u64>(nwords),
                     c.take<unsigned>(nwords), c.take<unsigned>(nwords), c.take<unsigned char>(nwords), c.take<unsigned>(blocks),
                     c.take<unsigned>(blocks), c.take<unsigned>(labels), c.take<unsigned>(labels), c.take<unsigned>(label_blocks),
                     c.take<unsigned>(label_blocks), c.take<u64>(2)};
}
// what the label sort of the emit call needs besides: sized by the totals the count call returned
constexpr int kSortBlock = 1024;          // items per workgroup of a radix pass: 4 waves x 4 rounds x 64 lanes
struct MeshLabelSortWs {
  u64* total;                     // the scan's grand total (two slots, not read)
  unsigned *vperm, *fperm;        // V / F: position of every raster-order item in label-major order
  unsigned short *vkey, *fkey;    // V / F: the label of every raster-order item
  unsigned short* key2;           // max(V, F): keys after the first of two passes
  unsigned* idx2;                 //            and the raster index they came from
  unsigned* hist;                 // 256 digits x sort blocks, digit-major; scanned in place
  unsigned* hblk;                 // block totals of that scan
};
static inline MeshLabelSortWs mesh_label_sort_ws(WsCarver& c, long long nverts, long long nfaces) {
  const size_t v = (size_t)nverts, f = (size_t)nfaces, m = std::max(v, f);
  const size_t bins = 256 * ((m + kSortBlock - 1) / kSortBlock);
  return MeshLabelSortWs{c.take<u64>(2), c.take<unsigned>(v), c.take<unsigned>(f), c.take<unsigned short>(v),
                         c.take<unsigned short>(f), c.take<unsigned short>(m), c.take<unsigned>(m), c.take<unsigned>(bins),
                         c.take<unsigned>((bins + kScanBlock - 1) / kScanBlock)};
}
size_t mesh_label_workspace_bytes(int n0, int n1, int n2);
size_t mesh_label_sort_bytes(long long nverts, long long nfaces);
// count: label check, count, scans; synchronises once to return the totals, the label count and the status.  vert_ptr_dev /
// face_ptr_dev: ptr_capacity device int64 each, entry k = items of the labels 1 .. k.  emit: verts and faces in label order.
int launch_mesh_label_count(const int* labels, int n0, int n1, int n2, int num, long long* nverts, long long* nfaces, int* num_used,
                            int* status, long long* vert_ptr_dev, long long* face_ptr_dev, int ptr_capacity, void* workspace,
                            size_t ws_bytes, hipStream_t s);
int launch_mesh_label_emit(const int* labels, int n0, int n1, int n2, int num, double level, long long nverts, long long nfaces,
                           float* verts, int* faces, const void* workspace, size_t ws_bytes, void* sort_workspace, size_t sort_bytes,
                           hipStream_t s);

// ---- branch morphometry (morphometry.hip): per-label integer tables of a parsing volume, its skeleton and the squared EDT -----
// Device arrays indexed by label value 0 .. num (include/seunet_hip.h, seunet_branch_stats).  No workspace: the tables are the
// only memory the passes write.
struct BranchStatsOut {
  long long *voxels, *coord_sum;            // [num + 1], [num + 1][3]
  int *box_min, *box_max;                   // [num + 1][3] each
  long long *skeleton_voxels, *links, *cross_links, *r2_sum;   // [num + 1], [num + 1][13], [num + 1][13], [num + 1]
  int *r2_min, *r2_max;                     // [num + 1] each
  int* status;
};
int launch_branch_stats(const int* parsing, const unsigned char* skeleton, const int* sqdist, int n0, int n1, int n2, int num,
                        BranchStatsOut out, hipStream_t s);
// the distance from the skeleton to the wall per label, from the feature transform of the EDT with spacing (edt_sampling.hip)
struct BranchWallOut {
  long long *wall_count, *offset_sq_sum;    // [num + 1], [num + 1][3]
  double *wall_sq_min, *wall_sq_max;        // [num + 1] each, reduced as their 64-bit patterns
  int* status;
};
int launch_branch_wall_stats(const int* parsing, const unsigned char* skeleton, const int* indices, int n0, int n1, int n2, int num,
                             double s0, double s1, double s2, BranchWallOut out, hipStream_t s);

// ---- airway cross-sections (cross_section.hip): the lumen section perpendicular to the centreline at every labelled skeleton voxel --
struct CrossRec { u64 total[2]; int status, pad; };   // what the host reads once: the scan's grand total, the label status
struct CrossWs {
  CrossRec* rec;
  u64* bits;                      // the point mask: one word per 64 voxels in raster order (not per row)
  unsigned* cnt;                  // per word: points, then their exclusive scan inside a block of 1024 words
  unsigned* blk;                  // per block: its total, then the exclusive scan of the totals
};
static inline CrossWs cross_section_ws(WsCarver& c, int n0, int n1, int n2) {
  const size_t nwords = ((size_t)n0 * n1 * n2 + 63) / 64, blocks = (nwords + kScanBlock - 1) / kScanBlock;
  return CrossWs{c.take<CrossRec>(1), c.take<u64>(nwords), c.take<unsigned>(nwords), c.take<unsigned>(blocks)};
}
size_t cross_section_workspace_bytes(int n0, int n1, int n2);
int cross_section_sweep_points();         // points one grid sweep of the section pass takes (one wave each)
// count: mark, scan; synchronises once to return the number of points and the label status (1: a label outside 0 .. num).
// emit: lin (m int32), tangent (m x 3 float64) and table (m x 12 int32) from the same workspace; does not synchronise.
int launch_cross_section_count(const int* parsing, const unsigned char* skeleton, int n0, int n1, int n2, int num, long long* m, int* status,
                               void* workspace, size_t ws_bytes, hipStream_t s);
int launch_cross_section_emit(const int* parsing, const unsigned char* skeleton, int n0, int n1, int n2, double s0, double s1, double s2,
                              double step, int window, int same_label, long long m, int* lin, double* tangent, int* table,
                              const void* workspace, size_t ws_bytes, hipStream_t s);

// ---- airway walls (airway_wall.hip): 64 FWHM rays in the section plane of every centreline point, one wave per point ------------
int airway_wall_rays();
int airway_wall_samples();
int airway_wall_sweep_points();           // points one grid sweep takes (one wave each)
void airway_wall_directions(double* out); // the committed table: (C_r, S_r) for r = 0 .. 63
// one launch, no workspace, no synchronise; table / tangent: the rows of launch_cross_section_emit; codes and edges may be null
int launch_airway_walls(const void* ct, int ct_dtype, const int* parsing, int n0, int n1, int n2, double s0, double s1, double s2,
                        double step, double ray_step, int n_search, float min_contrast, int same_label, long long m, const int* table,
                        const double* tangent, unsigned long long* mask, double* sums, unsigned char* codes, double* edges,
                        hipStream_t s);

// ---- soft skeleton / soft clDice loss / hard clDice counts (cldice.hip) -----------------------------------------------------
// `volumes` independent (n0, n1, n2) volumes back to back; n = volumes n0 n1 n2 voxels.  A forward that keeps no state needs
// the two E buffers only.  A saving forward (the loss's prediction branch) also fills the chains the backward reads; the
// backward writes `a` and reuses e0 / e1 for its running gradient, so the saved state survives it.
constexpr int kCldiceMaxIters = 16;
struct CldiceWs {
  float *e0, *e1;         // E_{j+1} of odd / even j (forward); dL/dE_j in turn (backward)
  float* d;               // iters + 1 volumes: d_j = relu(E_j - O_j)
  float* s;               // iters volumes: S_0 .. S_{iters-1} (S_iters is the forward's output)
  float* a;               // iters + 1 volumes: dL/dd_j, masked (backward)
  unsigned char* code;    // iters + 1 volumes: arg-min of E_{j+1} (bits 0-2), arg-max of O_j (bits 3-7)
};
static inline CldiceWs cldice_ws(WsCarver& c, long long volumes, int n0, int n1, int n2, int iters, bool save) {
  const size_t n = (size_t)volumes * n0 * n1 * n2, k = save ? (size_t)iters + 1 : 0;
  return CldiceWs{c.take<float>(n), c.take<float>(n), c.take<float>(k * n), c.take<float>(save ? (size_t)iters * n : 0),
                  c.take<float>(k * n), c.take<unsigned char>(k * n)};
}
size_t cldice_workspace_bytes(long long volumes, int n0, int n1, int n2, int iters, bool save);
int cldice_partial_doubles();
int launch_soft_skeleton(const float* x, long long volumes, int n0, int n1, int n2, int iters, float* out, bool save, void* workspace,
                         size_t ws_bytes, hipStream_t s);
int launch_cldice_sums(const float* sp, const float* t, const float* st, const float* p, long long n, double* partial, double* sums,
                       hipStream_t s);
int launch_cldice_value(const double* sums, double smooth, float* value, double* scal, hipStream_t s);
int launch_cldice_backward(const float* t, const float* st, const double* sums, double smooth, const float* g_dev, long long volumes,
                           int n0, int n1, int n2, int iters, float* grad, void* workspace, size_t ws_bytes, hipStream_t s);
int launch_cldice_counts(const unsigned char* sp, const unsigned char* vl, const unsigned char* sl, const unsigned char* vp, long long n,
                         unsigned long long* counts, hipStream_t s);

// ---- surface distances (surface.hip): border extraction, distances in raster order, their summary, order statistics -----------
constexpr int kSurfaceMaxTol = 8;         // tolerances per summary call
constexpr int kSelectMaxRanks = 8;        // requests per select call
struct SurfaceRec {                       // what the host reads once
  u64 n_a, n_b;                           // border voxels of A and of B: the scan's two totals
  int hi[3], from_end[3];                 // box of A | B as maxima: exclusive high end, extent - low end; all 0 = empty
};
struct SurfaceWs {
  SurfaceRec* rec;
  u64 *bits_a, *bits_b;                   // the packed masks; rows of ceil(n2 / 64) words, zero tails
  u64 *border_a, *border_b;               // their border voxels
  unsigned *cnt_a, *cnt_b;                // per word: border voxels, then their exclusive scan inside a block of 1024 words
  unsigned *blk_a, *blk_b;                // per block: its total, then the exclusive scan of the totals
};
static inline SurfaceWs surface_ws(WsCarver& c, int n0, int n1, int n2) {
  const size_t nwords = words(n0, n1, n2), blocks = (nwords + kScanBlock - 1) / kScanBlock;
  return SurfaceWs{c.take<SurfaceRec>(1), c.take<u64>(nwords), c.take<u64>(nwords), c.take<u64>(nwords), c.take<u64>(nwords),
                   c.take<unsigned>(nwords), c.take<unsigned>(nwords), c.take<unsigned>(blocks), c.take<unsigned>(blocks)};
}
struct SurfaceEmitWs {                    // on the extents of the box; used by one direction after the other
  unsigned char* sites;                   // 0 at the other mask's border voxels, 1 elsewhere: the EDT's input
  int* lin;                               // linear index in the box of every voxel's feature
  EdtSamplingWs edt;                      // one whole workspace of the EDT with spacing: edt_bytes from edt.f0 on
  size_t edt_bytes;
};
static inline SurfaceEmitWs surface_emit_ws(WsCarver& c, int b0, int b1, int b2) {
  const size_t n = (size_t)b0 * b1 * b2;
  SurfaceEmitWs w;
  w.sites = c.take<unsigned char>(n);
  w.lin = c.take<int>(n);
  w.edt_bytes = edt_sampling_workspace_bytes(b0, b1, b2);
  WsCarver edt(c.take<unsigned char>(w.edt_bytes));
  w.edt = edt_sampling_ws(edt, b0, b1, b2);
  return w;
}
struct SelectState { u64 prefix[kSelectMaxRanks], rank[kSelectMaxRanks]; };   // per request: digits chosen so far, rank among the rest
struct SelectWs {
  SelectState* state;
  unsigned* hist;                         // nranks x 256: this pass's digit histogram of every request
};
static inline SelectWs select_ws(WsCarver& c, int nranks) { return SelectWs{c.take<SelectState>(1), c.take<unsigned>((size_t)nranks * 256)}; }
size_t surface_workspace_bytes(int n0, int n1, int n2);
size_t surface_emit_workspace_bytes(int b0, int b1, int b2);
size_t surface_summary_bytes(int ntol);
size_t select_ranks_workspace_bytes(int nranks);
// count: pack, borders, counts, box, scan; synchronises once to return the totals and the box {lo0, hi0, lo1, hi1, lo2, hi2}.
// emit: dist[0 .. n_a) and dist[n_a .. n_a + n_b) (voxel: the same places, optional) from the count workspace, on the box.
int launch_surface_count(const unsigned char* a, const unsigned char* b, int n0, int n1, int n2, long long* n_a, long long* n_b, int* box,
                         void* workspace, size_t ws_bytes, hipStream_t s);
int launch_surface_emit(int n0, int n1, int n2, const int* box, double s0, double s1, double s2, long long n_a, long long n_b,
                        double* dist, int* voxel, const void* count_workspace, size_t count_bytes, void* emit_workspace, size_t emit_bytes,
                        hipStream_t s);
int launch_surface_summary(const double* dist, long long n_a, long long n_b, const double* tol, int ntol, void* out_dev, hipStream_t s);
int launch_select_ranks(const double* values, long long n, const long long* seg_begin, const long long* seg_end, const long long* rank,
                        int nranks, double* out_dev, void* workspace, size_t ws_bytes, hipStream_t s);

// ---- component labelling, Euler number, Betti numbers (betti.hip) -----------------------------------------------------------------
// connectivity 1 / 2 / 3 = 6 / 18 / 26 neighbours.  A patch (p0, p1, p2) cuts the volume into tiles from the origin (the last tile of
// an axis may be ragged); a tile's numbers are those of the tile cropped out as a volume of its own.  The whole volume is the one
// tile whose patch is the extents.
struct TileCut {
  int p0, p1, p2;         // patch extents, 1 .. n_k
  int t0, t1, t2;         // tiles per axis: ceil(n_k / p_k)
  long long tiles() const { return (long long)t0 * t1 * t2; }
};
static inline TileCut tile_cut(int n0, int n1, int n2, int p0, int p1, int p2) {
  p0 = std::min(std::max(p0, 1), n0); p1 = std::min(std::max(p1, 1), n1); p2 = std::min(std::max(p2, 1), n2);
  return TileCut{p0, p1, p2, (n0 + p0 - 1) / p0, (n1 + p1 - 1) / p1, (n2 + p2 - 1) / p2};
}
struct LabelWs {
  int* labels;            // minimum linear index of every voxel's component, -1 off (handed unchanged to the table call)
  unsigned* counts;       // voxels per root (the table call)
  u64* roots;             // the packed mask of the roots; rows of ceil(n2 / 64) words, zero tails
  unsigned* cnt;          // per word: roots, then their exclusive scan inside a block of 1024 words
  unsigned* blk;          // per block: its total, then the exclusive scan of the totals
  unsigned* base;         // words + 1: the plain exclusive scan; the last entry is the number of components
  u64* total;             // the scan's grand total (two slots)
};
static inline LabelWs label_ws(WsCarver& c, int n0, int n1, int n2) {
  const size_t n = (size_t)n0 * n1 * n2, nwords = words(n0, n1, n2), blocks = (nwords + kScanBlock - 1) / kScanBlock;
  return LabelWs{c.take<int>(n), c.take<unsigned>(n), c.take<u64>(nwords), c.take<unsigned>(nwords), c.take<unsigned>(blocks),
                 c.take<unsigned>(nwords + 1), c.take<u64>(2)};
}
constexpr int kCellClasses = 4;           // cell counts per tile, by the number of axes a cell spans two voxels along
struct EulerWs {
  u64* bits;              // the packed volume; rows of ceil(n2 / 64) words, zero tails
  u64* cells;             // tiles x kCellClasses
};
static inline EulerWs euler_ws(WsCarver& c, int n0, int n1, int n2, long long tiles) {
  return EulerWs{c.take<u64>(words(n0, n1, n2)), c.take<u64>((size_t)tiles * kCellClasses)};
}
struct BettiWs {
  int* labels;            // the foreground's labels, then the complement's
  unsigned char* flag;    // per root of the complement: 1 = its component reaches a face of its tile
  EulerWs euler;
};
static inline BettiWs betti_ws(WsCarver& c, int n0, int n1, int n2, long long tiles) {
  const size_t n = (size_t)n0 * n1 * n2;
  BettiWs w;
  w.labels = c.take<int>(n);
  w.flag = c.take<unsigned char>(n);
  w.euler = euler_ws(c, n0, n1, n2, tiles);
  return w;
}
size_t label_workspace_bytes(int n0, int n1, int n2);
size_t euler_workspace_bytes(int n0, int n1, int n2, TileCut t);
size_t betti_workspace_bytes(int n0, int n1, int n2, TileCut t);
// labels_out: 0 off, 1 .. N in raster order of each component's first voxel; num_dev (optional): N.  Does not synchronise.
int launch_label(const unsigned char* vol, int n0, int n1, int n2, int connectivity, int* labels_out, int* num_dev, void* workspace,
                 size_t ws_bytes, hipStream_t s);
// size / first (num int64 each) and box (num x {min0, max0, min1, max1, min2, max2}) from the label call's output and workspace
int launch_component_table(const int* labels, int n0, int n1, int n2, long long num, long long* size, long long* first, int* box,
                           void* workspace, size_t ws_bytes, hipStream_t s);
// out = the voxels of the components with at least min_size voxels; workspace: cc_ws
int launch_remove_small(const unsigned char* vol, int n0, int n1, int n2, long long min_size, int connectivity, unsigned char* out,
                        void* workspace, size_t ws_bytes, hipStream_t s);
// chi_dev: one int64 per tile, raster tile order
int launch_euler(const unsigned char* vol, int n0, int n1, int n2, TileCut t, int connectivity, long long* chi_dev, void* workspace,
                 size_t ws_bytes, hipStream_t s);
// table_dev: int32 (tiles, 3) = (b0, b1, b2) per tile, raster tile order
int launch_betti(const unsigned char* vol, int n0, int n1, int n2, TileCut t, int connectivity, int* table_dev, void* workspace,
                 size_t ws_bytes, hipStream_t s);

// ---- device helpers -------------------------------------------------------------------------------------------------------
// raster index -> coordinates of an (n0, n1, n2) volume (n0 is not needed)
struct Vox3 { int i0, i1, i2; };
__device__ __forceinline__ Vox3 vox3(long long i, int n1, int n2) {
  const int i2 = (int)(i % n2);
  const long long r = i / n2;
  Vox3 p;
  p.i1 = (int)(r % n1);
  p.i0 = (int)(r / n1);
  p.i2 = i2;
  return p;
}

// non-zero voxels of the 3x3x3 block around p, centre included, with indices clamped to the volume: scipy's mode 'reflect' at
// radius 1 repeats the edge voxel (index -1 -> 0, n -> n - 1), so a voxel on a face counts itself and its in-face neighbours twice
__device__ __forceinline__ int count27_clamped(const unsigned char* __restrict__ vol, Vox3 p, int n0, int n1, int n2) {
  int cnt = 0;
  for (int a = -1; a <= 1; ++a)
    for (int b = -1; b <= 1; ++b) {
      const int x0 = std::min(std::max(p.i0 + a, 0), n0 - 1), x1 = std::min(std::max(p.i1 + b, 0), n1 - 1);
      const unsigned char* row = vol + ((long long)x0 * n1 + x1) * n2;
      for (int c = -1; c <= 1; ++c) cnt += row[std::min(std::max(p.i2 + c, 0), n2 - 1)] != 0;
    }
  return cnt;
}

// maximum over the 64 lanes, in every lane
template <typename V> __device__ __forceinline__ V wave_max(V v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const V o = shfl_xor_settled(v, off);
    v = o > v ? o : v;
  }
  return v;
}
// sum over the 64 lanes, in every lane: the butterfly 32, 16, .. 1, so a floating-point sum is a tree of one fixed shape
template <typename V> __device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += shfl_xor_settled(v, off);
  return v;
}

}  // namespace seunet
