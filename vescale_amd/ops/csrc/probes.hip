// Hardware layout probes and their bindings (decoded by tools/fa_fwd_check.py,
// tools/permlane_probe.py, tools/tr_probe_check.py; the relayout probe by
// tests/test_fa32_tile_paths_gpu.py).  Included by extension.hip
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

// ff_relayout's earlier formulation, kept for the relayout probe ONLY: every
// packed word exchanged with the one-operand swap (ff_swap_other, which picks
// the partner's copy with a select), the fragment then assembled with a second
// select on `half`: 16 swaps and 32 selects per tile against ff_relayout's 8
// swaps.  The probe holds ff_relayout to this one's bits.
DEV void ff_relayout_ref(const ff_floatx16 st[2], ff_shortx8 pb[4], int half) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const unsigned lo0 = ff_cvt_pk(st[s2][g * 8 + 0], st[s2][g * 8 + 1]);
      const unsigned lo1 = ff_cvt_pk(st[s2][g * 8 + 2], st[s2][g * 8 + 3]);
      const unsigned hi0 = ff_cvt_pk(st[s2][g * 8 + 4], st[s2][g * 8 + 5]);
      const unsigned hi1 = ff_cvt_pk(st[s2][g * 8 + 6], st[s2][g * 8 + 7]);
      int p0 = ff_swap_other((int)lo0, half);  // partner's LO word0
      int p1 = ff_swap_other((int)lo1, half);  // partner's LO word1
      int p2 = ff_swap_other((int)hi0, half);  // partner's HI word0
      int p3 = ff_swap_other((int)hi1, half);  // partner's HI word1
      ff_intx4 frag;
      if (half == 0) {
        frag = (ff_intx4){(int)lo0, (int)lo1, p0, p1};
      } else {
        frag = (ff_intx4){p2, p3, (int)hi0, (int)hi1};
      }
      pb[s2 * 2 + g] = *reinterpret_cast<ff_shortx8*>(&frag);
    }
  }
}

// relayout probe: one wave; lane l reads its 2 x 16 fp32 D-layout registers
// from in[l][32] and writes the 4 fragments of ff_relayout_ref to
// out[0][l][4][8] and those of ff_relayout to out[1][l][4][8] (bf16 bits).
extern "C" __global__ void relayout_probe_kernel(const float* __restrict__ in,
                                                 unsigned short* __restrict__ out) {
  const int lane = threadIdx.x;  // one wave
  ff_floatx16 st[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int r = 0; r < 16; ++r) st[s2][r] = in[lane * 32 + s2 * 16 + r];
  ff_shortx8 ref[4], got[4];
  ff_relayout_ref(st, ref, lane >> 5);
  ff_relayout(st, got);
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    *reinterpret_cast<ff_shortx8*>(out + ((0 * 64 + lane) * 4 + f) * 8) = ref[f];
    *reinterpret_cast<ff_shortx8*>(out + ((1 * 64 + lane) * 4 + f) * 8) = got[f];
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

// x: [64, 32] fp32 (lane, s2*16 + r) -> [2 (ref, new), 64, 4, 8] bf16 bits
at::Tensor relayout_probe(at::Tensor x) {
  Binding b("_relayout_probe", "x", x);
  b.arg("x", x, F32, {64, 32});
  auto out = at::empty({2, 64, 4, 8}, x.options().dtype(at::kShort));  // on x's device
  b.launch(relayout_probe_kernel, 1, 64, x.data_ptr<float>(), bf16_mut(out));
  return out;
}

}  // namespace
