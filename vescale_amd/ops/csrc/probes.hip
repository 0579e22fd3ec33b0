// Hardware layout probes and their bindings (decoded by tools/fa_fwd_check.py,
// tools/permlane_probe.py, tools/tr_probe_check.py).  Included by extension.hip
// after the host helpers (Binding); the device helpers it probes come from
// fa32_common.h.
#include "fa32_common.h"

extern "C" __global__ void permlane_probe_kernel(int* out) {
  int x = (int)threadIdx.x;
  auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  out[threadIdx.x] = (r[0] << 16) | (r[1] & 0xFFFF);
}

// mfma_f32_32x32x16_bf16 layout probe: builds A/B frags per the ASSUMED
// layout (operand row/col = lane&31, k = (lane>>5)*8 + e) and dumps D for
// three tests; see tools/fa_fwd_check.py for decoding.
extern "C" __global__ void mfma32_probe_kernel(float* out) {
  typedef short sx8 __attribute__((ext_vector_type(8)));
  typedef float fx16 __attribute__((ext_vector_type(16)));
  int lane = threadIdx.x & 63;
  int l31 = lane & 31, half = lane >> 5;
  sx8 af, bf, a1, bj, ak, bk;
  for (int e = 0; e < 8; ++e) {
    int k = half * 8 + e;
    af[e] = (short)f32_to_bf16((float)((k == 0) ? l31 : 0));
    bf[e] = (short)f32_to_bf16((float)((k == 0) ? 1 : 0));
    a1[e] = bf[e];
    bj[e] = (short)f32_to_bf16((float)((k == 0) ? l31 : 0));
    ak[e] = (short)f32_to_bf16((float)((k == 5) ? 1 : 0));
    bk[e] = (short)f32_to_bf16((float)((k == 5) ? l31 : 0));
  }
  fx16 z = (fx16)(0.f);
  fx16 d1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, z, 0, 0, 0);
  fx16 d2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bj, z, 0, 0, 0);
  fx16 d3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ak, bk, z, 0, 0, 0);
  for (int r = 0; r < 16; ++r) {
    out[0 * 64 * 16 + lane * 16 + r] = d1[r];
    out[1 * 64 * 16 + lane * 16 + r] = d2[r];
    out[2 * 64 * 16 + lane * 16 + r] = d3[r];
  }
}

// tr-read addressing probe for the 4x4-group transpose scheme: stage a
// pattern (value = kv*128 + d) through the kernels' swizzled staging store
// (ff_chunk_store), then read it back with the kernels' tr-read function
// (ff_tr_read8); host checks lane l elem
// e == (ks*16 + half*8 + e)*128 + ds*32 + l31 (tools/tr_probe_check.py).
extern "C" __global__ void tr_probe_kernel(unsigned short* out) {
  __shared__ unsigned short lvp[64 * FF_D];
  const int lane = threadIdx.x;  // one wave
#pragma unroll
  for (int j = 0; j < FF_STAGE_CHUNKS(64, 64); ++j) {
    const int e = ff_chunk<64>(j, lane);
    ff_shortx8 vv;
#pragma unroll
    for (int x = 0; x < 8; ++x) vv[x] = (short)(e + x);
    ff_chunk_store(vv, lvp, e);
  }
  __syncthreads();
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) {
    ff_shortx4 t[4][2];
    ff_tr_read8(lvp, ds, lane, lane & 31, lane >> 5, t);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      *reinterpret_cast<ff_shortx8*>(out + ((ds * 4 + ks) * 64 + lane) * 8) =
          ff_cat(t[ks][0], t[ks][1]);
  }
}

namespace {

at::Tensor probe_out(at::IntArrayRef sizes, at::ScalarType dtype) {
  return at::empty(sizes, at::TensorOptions().dtype(dtype).device(at::kCUDA));
}

at::Tensor permlane_probe() {
  auto out = probe_out({64}, at::kInt);
  Binding("permlane_probe", "out", out).launch(permlane_probe_kernel, 1, 64, out.data_ptr<int>());
  return out;
}

at::Tensor mfma32_probe() {
  auto out = probe_out({3, 64, 16}, at::kFloat);
  Binding("mfma32_probe", "out", out).launch(mfma32_probe_kernel, 1, 64, out.data_ptr<float>());
  return out;
}

at::Tensor tr_probe() {
  auto out = probe_out({4, 4, 64, 8}, at::kShort);
  Binding("tr_probe", "out", out).launch(tr_probe_kernel, 1, 64, bf16_mut(out));
  return out;
}

}  // namespace
