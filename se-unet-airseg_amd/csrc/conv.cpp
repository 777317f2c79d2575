// The forward / data-gradient convolution family by kernel (conv.h): the only switches over ConvKernel on this side.
#include "conv.h"
#include "epilogue.h"

#include <vector>

namespace seunet {

bool conv_supported(ConvKernel k, int dtype, int taps, int dil, const SrcList& src, const DstList& dst) {
  switch (k) {
    case ConvKernel::Stream: return src.n == 1 && dst.n == 1 && conv_stream_supported(dtype, taps, dil, src.C[0], dst.C[0]);
    case ConvKernel::March: return conv_march_supported(dtype, taps, dil, src, dst);
    default: return k == ConvKernel::Tiled || k == ConvKernel::Naive;
  }
}

size_t conv_wpack_bytes(ConvKernel k, int dtype, int taps, int src_c, int cin, int cout) {
  switch (k) {
    case ConvKernel::Stream: return conv_stream_wpack_bytes(src_c);
    case ConvKernel::March: return conv_march_wpack_bytes(cin, cout);
    default: return conv_igemm_wpack_bytes(dtype, taps, cin, cout);   // (the naive kernels read the PyTorch weight: same slot)
  }
}

int conv_slots(ConvKernel k, Dims d, int taps, int dil, int cin, int cout) {
  switch (k) {
    case ConvKernel::Stream: return conv_stream_slots(d, dil);
    case ConvKernel::March: return conv_march_slots(d, dil, cin, cout);
    case ConvKernel::Naive: return epi_partials(d);
    default: return conv_stats_tiles(d, taps, dil);
  }
}

int run_conv(ConvKernel k, int dtype, int taps, int dil, const SrcList& src, int cin_logical, const float* w_torch, int tflip,
             const void* wpack, const float* bias, const DstList& dst, double* stats, Dims d, hipStream_t s) {
  switch (k) {
    case ConvKernel::Naive: return launch_conv_naive(dtype, taps, dil, src, cin_logical, w_torch, tflip, bias, dst, d, s);
    case ConvKernel::Tiled: return launch_conv_igemm(dtype, taps, dil, src, cin_logical, wpack, bias, dst, stats, d, s);
    case ConvKernel::Stream:
      return launch_conv_stream(dtype, dil, src.ptr[0], src.C[0], wpack, bias, dst.ptr[0], dst.C[0], dst.acc[0], stats, d, s);
    case ConvKernel::March: return launch_conv_march(dtype, dil, src, wpack, bias, dst, stats, d, s);
    default: return fail("net: internal: kernel %d runs no convolution", (int)k);
  }
}

int launch_conv_pack(int dtype, const ConvPackJob* jobs, int n, hipStream_t s) {
  struct { ConvKernel k; int (*launch)(int, const ConvPackJob*, int, hipStream_t); } const order[] = {
      {ConvKernel::Stream, launch_conv_stream_pack}, {ConvKernel::March, launch_conv_march_pack}, {ConvKernel::Tiled, launch_conv_igemm_pack}};
  std::vector<ConvPackJob> group;
  for (const auto& o : order) {
    group.clear();
    for (int i = 0; i < n; ++i)
      if (jobs[i].k == o.k) group.push_back(jobs[i]);
    if (int e = o.launch(dtype, group.data(), (int)group.size(), s)) return e;
  }
  return 0;
}

}  // namespace seunet
