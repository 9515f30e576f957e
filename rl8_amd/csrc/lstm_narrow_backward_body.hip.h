// The body of lstm_narrow_backward_kernel<H> and lstm_narrow_backward_heads_kernel<H> (lstm_narrow_kernels.hip), included
// inside each kernel's braces after `constexpr bool HEADS` and the pointers the variant does not take (dhs, or heads_dout
// and heads_w) have been declared.  Text, not a __device__ function: the compiler schedules an inlined body differently
// from a kernel's own, and the plain kernel's code must stay what it was, instruction for instruction.
//
// HEADS: dL/dh_t is not read from dhs but formed from the output heads it came through, dh[b][t][u] = sum_q
// heads_dout[b][t][q] heads_w[q][u], q < 4 (zero-padded): the lane holds its unit's four weights; a step's floats are
// loaded behind the barrier that precedes the recurrent product of the step after it (in time: t - 1), where no gate
// is in flight, and folded into the carry when the product is done -- the same sum, in the same order, as
// dhs + carry with dhs formed by linear_heads_narrow_backward_kernel.
  using G = Geo<H>;
  constexpr int MT = G::MTB, R = G::RB, LD = G::LD;
  extern __shared__ float lds[];  // [R][LD]: dz of the step
  const int tid = threadIdx.x, lane = tid & 63, qq = lane >> 4, l16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int u = 16 * wave + l16;

  // B operand of dh_{t-1} = dz x W_hh: wt[4g + e] = W_hh[16g + 4qq + e][u], k over the 4H gate columns.
  float wt[H];
#pragma unroll
  for (int g = 0; g < H / 4; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) wt[4 * g + e] = w_hh[(int64_t)(16 * g + 4 * qq + e) * H + u];
  const int v_state = (4 * qq * H + u) * 4, v_seq = (4 * qq * l * H + u) * 4, v_gates = (4 * qq * l * 4 * H + u) * 4;
  const int v_heads = (4 * qq * l * 4 + (l16 & 3)) * 4;  // HEADS: lane part of the offset into heads_dout [rows][l][4]
  float hw[4];  // HEADS: heads_w[q][u]
  if constexpr (HEADS) {
#pragma unroll
    for (int q = 0; q < 4; ++q) hw[q] = heads_w[q * H + u];
  }

  const int64_t tiles = (b + R - 1) / R;
  for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
    const int64_t b0 = ti * R;
    float dh_carry[MT][4], dc_carry[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) dh_carry[mt][r] = dc_carry[mt][r] = 0.0f;
    // (buffer descriptors as in the forward: rows past b read 0 and drop their stores)
    const int rows = (int)(b - b0 < R ? b - b0 : R);
    const uint32_t span = (uint32_t)((rows - 1) * l + 1) * 4;
    const __amdgpu_buffer_rsrc_t c0r = buffer_rsrc(c0 + b0 * H, (uint32_t)rows * H * 4);
    // HEADS: the tile's rows of heads_dout [b][l][4] at step t.  A row's 16 bytes are shared by the 16 lanes of its
    // units: lane l16 loads float l16 & 3 of each of its rows (one register per row in flight, not four), and the
    // four floats of a row come back through quad broadcasts (DPP) when dh is formed.  (The whole offset in the
    // VGPR, which the range check covers.)
    float hd[MT][4];
    auto heads_fetch = [&](int t) {
      const __amdgpu_buffer_rsrc_t hr = buffer_rsrc(heads_dout + (b0 * l + t) * 4, span * 4);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) hd[mt][r] = buffer_load_f32(hr, v_heads + (16 * mt + r) * l * 16, 0);
    };
    auto heads_dh = [&](float d) {
      const int di = __builtin_bit_cast(int, d);
      float g = 0.0f;
      g = __builtin_fmaf(__builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, di, 0x00, 0xf, 0xf, false)), hw[0], g);
      g = __builtin_fmaf(__builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, di, 0x55, 0xf, 0xf, false)), hw[1], g);
      g = __builtin_fmaf(__builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, di, 0xaa, 0xf, 0xf, false)), hw[2], g);
      g = __builtin_fmaf(__builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, di, 0xff, 0xf, 0xf, false)), hw[3], g);
      return g;
    };
    if constexpr (HEADS) {
      heads_fetch(l - 1);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dh_carry[mt][r] = heads_dh(hd[mt][r]);
    }
    for (int t = l - 1; t >= 0; --t) {
      const int64_t rs0 = b0 * l + t;
      const __amdgpu_buffer_rsrc_t gr = buffer_rsrc(gates + rs0 * 4 * H, span * 4 * H);
      const __amdgpu_buffer_rsrc_t zr = buffer_rsrc(dz + rs0 * 4 * H, span * 4 * H);
      const __amdgpu_buffer_rsrc_t cr = buffer_rsrc(cs + rs0 * H, span * H);
      const __amdgpu_buffer_rsrc_t cpr = buffer_rsrc(cs + (t > 0 ? rs0 - 1 : 0) * H, span * H);
      const __amdgpu_buffer_rsrc_t dr = buffer_rsrc(HEADS ? nullptr : dhs + rs0 * H, span * H);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int sr = 16 * mt + r, so_g = sr * l * 4 * H * 4, so_s = sr * l * H * 4;
          const float ig = buffer_load_f32(gr, v_gates + so_g, 0), fg = buffer_load_f32(gr, v_gates + so_g + H * 4, 0);
          const float gg = buffer_load_f32(gr, v_gates + so_g + 2 * H * 4, 0);
          const float og = buffer_load_f32(gr, v_gates + so_g + 3 * H * 4, 0);
          const float ct = buffer_load_f32(cr, v_seq + so_s, 0);
          const float cp = t > 0 ? buffer_load_f32(cpr, v_seq + so_s, 0) : buffer_load_f32(c0r, v_state + sr * H * 4, 0);
          float dh;
          if constexpr (HEADS) dh = dh_carry[mt][r];  // (the heads' part went into the carry)
          else dh = buffer_load_f32(dr, v_seq + so_s, 0) + dh_carry[mt][r];
          const float tc = tanh_f(ct);
          const float d_o = dh * tc * (og * (1.0f - og));
          const float dc = __builtin_fmaf(dh * og, 1.0f - tc * tc, dc_carry[mt][r]);
          const float d_i = dc * gg * (ig * (1.0f - ig));
          const float d_g = dc * ig * (1.0f - gg * gg);
          const float d_f = dc * cp * (fg * (1.0f - fg));
          dc_carry[mt][r] = dc * fg;
          buffer_store_f32(d_i, zr, v_gates + so_g, 0);
          buffer_store_f32(d_f, zr, v_gates + so_g + H * 4, 0);
          buffer_store_f32(d_g, zr, v_gates + so_g + 2 * H * 4, 0);
          buffer_store_f32(d_o, zr, v_gates + so_g + 3 * H * 4, 0);
          float *zs = lds + (16 * mt + 4 * qq + r) * LD + u;
          zs[0] = d_i;
          zs[H] = d_f;
          zs[2 * H] = d_g;
          zs[3 * H] = d_o;
        }
      if (t == 0) break;  // (dh_{-1}: a gradient to h0, not formed)
      __syncthreads();  // the step's dz is complete
      if constexpr (HEADS) heads_fetch(t - 1);  // lands during the product
      f32x4 acc[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      f32x4 a[MT], an[MT];  // (read a group ahead, fenced: as in the forward)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f32x4 *>(lds + (16 * mt + l16) * LD + 4 * qq);
#pragma unroll
      for (int g = 0; g < H / 4; ++g) {
        if (g + 1 < H / 4) {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            an[mt] = *reinterpret_cast<const f32x4 *>(lds + (16 * mt + l16) * LD + 16 * (g + 1) + 4 * qq);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][e], wt[4 * g + e], acc[mt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = an[mt];
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (HEADS) dh_carry[mt][r] = heads_dh(hd[mt][r]) + acc[mt][r];
          else dh_carry[mt][r] = acc[mt][r];
        }
      __syncthreads();  // every wave has read the step's dz
    }
  }
