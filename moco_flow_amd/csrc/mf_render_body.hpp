// mf_render_body.hpp -- the body of the fp32 render kernels (mf_render.hip), included INSIDE each kernel definition: in scope are
// `RenderParams p` and the compile-time bools MOCO (NoF chains in front of the NeRF), DUMP (training forward) and FOLD (nerf_packed
// is the folded stream of mf_nerf_pack_fold, inference only).  A body and not a function template: render_kernel<MOCO, DUMP>
// keeps its names and compiles to the code it had before the folded kernels existed -- behind a forced-inline call the same
// source came out with another register allocation in all four instantiations.
// MF_BODY_FOLD (0 | 1, defined around the #include): the text of the folded kernels alone -- `p` is their FoldRenderParams there.
  const LaneId id;
  const NetDev nerf = p.nerf;
  const WgClock wg;
  load_resident(nerf, id);
  if (MOCO) {
    load_resident(p.bw, id);
    if (p.flags & (MF_F_CHAIN_LOCAL | MF_F_CHAIN_GLOBAL)) load_resident(p.fw, id);
  }
  emb_tables_to_lds<RenderParams>(p);
  const uint32_t par_nerf_xyz = p.par_off, par_nerf_ext = p.par_off + 128, par_nof_xyz = p.par_off + 256,
                 par_nof_ind = p.par_off + 384;
  Stream st;
  CarryT<kPD> carry;
  st.open(p.ring_off, p.buf_bytes, MF_TIMING_FLAGS ? p.dbg : 0);
  st.tl.start(p.alphas, id);
  // the panel program of a tile: [bw NoF, fw NoF chains,] NeRF, then around again
#if MF_BODY_FOLD   // (the NeRF-only folded kernel streams layer 0 in long panels: trunk_layer0_long, mf_nets.hpp; behind the NoF chains
                   //  the MoCo kernel keeps the short ones -- with long panels it spilled 7 VGPRs)
  const NextLayer prog_first = MOCO ? follow_of(p.bw) : follow_of_long(nerf);
  if (MOCO) start_program(p.bw, st, carry, id);
  else start_program_long(nerf, st, carry, id);
#else
  const NextLayer prog_first = MOCO ? follow_of(p.bw) : follow_of(nerf);
  if (MOCO) start_program(p.bw, st, carry, id);
  else start_program(nerf, st, carry, id);
#endif

  const int S = p.S;
  const bool sigma_only = p.flags & MF_F_SIGMA_ONLY;
  float4* sbuf = reinterpret_cast<float4*>(smem + p.sbuf_off);
  float* zbuf = reinterpret_cast<float*>(smem + p.zbuf_off);

  for (long long group = blockIdx.x; group < p.n_groups; group += gridDim.x) {
    const long long ray0 = group * p.G;
    const int nr = (int)((p.n_rays - ray0) < p.G ? (p.n_rays - ray0) : p.G);
    const int nsamp = nr * S;
    const int ntiles = (nsamp + kTile - 1) / kTile;

#if MF_BODY_FOLD
    {
      // The extra block of extra_encoding (rendering.py:133-142) is the same for every sample of a ray: once per group,
      //   row[r][o] = b'[o] + sum_k W_e[o, W + k] PE(ext_r)[k]      (fp32 fmaf from b', k ascending in the reference's column order)
      // for the group's rays, which the tiles' lanes take as their accumulators' initial value (nerf_eval's ray_bias).
      if (p.fold_wx) {
        const int t = threadIdx.x;
        const uint32_t rpe_off = p.rbias_off + (uint32_t)p.G * (kFoldHalf * 4);         // the encodings sit behind the G rows
        // (thread t's row o = t % (W/2) of W_e[:, W:], asked for first: the loads fly while the encodings are evaluated)
        const int o = t & (kFoldHalf - 1);
        f32x4 w4[kRayPeFloats / 4];
#pragma unroll
        for (int q = 0; q < kRayPeFloats / 4; ++q) {
          w4[q] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (4 * q < p.fold_xcols) w4[q] = *reinterpret_cast<const f32x4*>(p.fold_wx + o * p.fold_xcols + 4 * q);
        }
        // 1. the rays' encodings by the text the per-sample path evaluated: thread 4 r + g = lane group g's slots of ray r
        for (int r = t >> 2; r < nr; r += kThreads / 4) {
          const int g = t & 3;
          const float* rp = p.rays + (ray0 + r) * p.ray_stride;
          float e[kStepsExtraMax];
#pragma unroll
          for (int s = 0; s < kStepsExtraMax; ++s) e[s] = 0.f;
          const bool dir = p.extra_type == MF_EXTRA_DIR;
          if (dir) {
            const float dd[3] = {rp[3], rp[4], rp[5]};
            emb_eval_lds<3, 4>(e, dd, par_nerf_ext, g);                                  // rendering.py:138-142
          } else {
            const float iv[1] = {rp[8]};
            emb_eval_lds<1, 2>(e, iv, par_nerf_ext, g);                                  // rendering.py:133-137
          }
          float* pe = reinterpret_cast<float*>(smem + rpe_off) + r * kRayPeFloats;
          const int nfeat = dir ? 27 : 5;
#pragma unroll
          for (int s = 0; s < kStepsExtraMax; ++s) {
            const int f = emb_feature(dir ? kEmbDir : kEmbInd, g, s, 0);
            if (f >= 0) pe[f] = e[s];
          }
          for (int f = nfeat + g; f < kRayPeFloats; f += 4) pe[f] = 0.f;
        }
        __syncthreads();
        // 2. thread (o = t % (W/2), r = t / (W/2) + 4 i): its weight row from registers, the encodings by broadcast reads
        const float b = lds_f(nerf.res_lds + (nerf.L.off_bias_extra + o) * 4);
        for (int r = t / kFoldHalf; r < nr; r += kThreads / kFoldHalf) {
          float acc = b;
#pragma unroll
          for (int q = 0; q < kRayPeFloats / 4; ++q) {
            const f32x4 e4 = lds_f4(rpe_off + (r * kRayPeFloats + 4 * q) * 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = __builtin_fmaf(w4[q][i], e4[i], acc);
          }
          *reinterpret_cast<float*>(smem + p.rbias_off + (r * kFoldHalf + o) * 4) = acc;
        }
        // (published by the panel barriers in front of trunk layer D - 1's last panel, where the first row is read; the next
        //  group's phase runs behind this group's composite barriers)
      }
    }
#endif

    for (int tile = 0; tile < ntiles; ++tile) {
      st.tl.stamp(1, id);
      // Per-sample bookkeeping (sample / ray indices, the ray's row pointer, the index columns) is NOT carried through the
      // tile: everything follows from the lane's column j and tile-uniform scalars, so each use site rebuilds what it
      // needs from an opaque copy of j (`where()`).  Held in registers from here, those values -- and the 64-bit
      // addresses hipcc derives from them ahead of time -- were what the MoCo training forward spilled (12 registers, 116
      // bytes of scratch per lane in round 2's build).  z and the observation-space point wait in the group's LDS
      // sample buffers (their slots are free until the tile's results are written).
      struct Where { int srel, sl, si; bool valid; long long ray; const float* rp; };
      auto where = [&]() {
        int jo = id.j;
        asm volatile("" : "+v"(jo));
        Where w;
        w.srel = tile * kTile + id.wave * kWaveSamples + jo;
        w.valid = w.srel < nsamp;
        w.sl = w.valid ? w.srel : nsamp - 1;
        const int rr = w.sl / S;
        w.si = w.sl - rr * S;
        w.ray = ray0 + rr;
        w.rp = p.rays + w.ray * p.ray_stride;
        return w;
      };
      float xin[3];                            // what the canonical NeRF sees
      {
        const Where w = where();
        const float* rp = w.rp;
        const float o[3] = {rp[0], rp[1], rp[2]};
        const float d[3] = {rp[3], rp[4], rp[5]};
        const float z = ray_depth(p, rp, w.ray, w.si);
        ray_point(o, d, z, xin);
        if (w.valid && id.g == 0) {
          zbuf[w.srel] = z;
          if (MOCO) sbuf[w.srel] = make_float4(xin[0], xin[1], xin[2], 0.f);
        }
      }
#ifdef MF_TIMELINE
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(xin[0]), "+v"(xin[1]), "+v"(xin[2]));
#endif
      st.tl.stamp(2, id);
      if (MOCO) {
        // chain program (rendering.py:270-282), roles: mf_raypass.hpp
        const int nsteps = chain_steps(p.flags);
        float canon[3] = {0.f, 0.f, 0.f}, cur[3] = {xin[0], xin[1], xin[2]};
        for (int step = 0; step < nsteps; ++step) {
          const int role = step;
          const NetDev net = role_uses_fw(role) ? p.fw : p.bw;
          const Where w = where();
          const float ind = w.rp[role_ind_column(role)];
          if (role == 1 || role == 2) { cur[0] = canon[0]; cur[1] = canon[1]; cur[2] = canon[2]; }
          // what follows this evaluation in the panel program
          const bool last = step == nsteps - 1;
          const NextLayer follow = last ? follow_of(nerf) : (role_uses_fw(role + 1) ? follow_of(p.fw) : follow_of(p.bw));
          float emb[kStepsNofIn], out[3];
          nof_embed_lds(emb, cur, ind, par_nof_xyz, par_nof_ind, id.g);
          float* nof_row = nullptr;
          if constexpr (DUMP) {
            if (w.valid && p.dump_nof_acts) {
              // training forward: what autograd.NofPoints' backward reads, per chain step (step-major planes)
              const long long nof_idx = (long long)((p.nof_plane_pack >> (3 * step)) & 7u) * p.n_rays * S + (w.ray * S + w.si);
              nof_row = p.dump_nof_acts + nof_idx * p.dump_nof_stride;
              // embedded input in the kernel's own slot order (column 20 g + e = slot e of lane group g: five 16-byte
              // stores per lane instead of twenty scattered dwords; mf_nof_emb_slot_features gives the column map)
              float4* e4 = reinterpret_cast<float4*>(p.dump_nof_emb + nof_idx * 80 + 20 * id.g);
#pragma unroll
              for (int q = 0; q < kStepsNofIn / 4; ++q) e4[q] = make_float4(emb[4 * q], emb[4 * q + 1], emb[4 * q + 2], emb[4 * q + 3]);
            }
            st.keep2 = 0;
          }
          nof_eval<DUMP>(net, emb, cur, st, carry, id, follow, out, nof_row,
                         DUMP && p.dump_nof_stride >= (long long)net.L.n_trunk * net.L.W + 16 + 4 * net.L.n_trunk);
          if constexpr (DUMP) {
            const Where v = where();
            if (v.valid && p.dump_nof_acts && id.g == 0) {
              const long long nof_idx = (long long)((p.nof_plane_pack >> (3 * step)) & 7u) * p.n_rays * S + (v.ray * S + v.si);
              float* q = p.dump_nof_out + nof_idx * 3;
              q[0] = out[0]; q[1] = out[1]; q[2] = out[2];
            }
          }
          if (role == 0) { canon[0] = out[0]; canon[1] = out[1]; canon[2] = out[2]; }
          if (role == 1 || role == 4) {
            const Where v = where();
            const float4 x4 = sbuf[v.sl];          // the observation-space point (own wave's write, or -- lanes past the
                                                   // group's last sample -- anything: their distances are never stored)
            const float dd = (fabsf(x4.x - out[0]) + fabsf(x4.y - out[1]) + fabsf(x4.z - out[2])) / 3.f;
            float* plane = role == 1 ? p.disp_local : p.disp_global;       // rendering.py:310-314, stored right away
            if (v.valid && id.g == 0 && plane) plane[v.ray * S + v.si] = dd;
          }
          cur[0] = out[0]; cur[1] = out[1]; cur[2] = out[2];
        }
        xin[0] = canon[0]; xin[1] = canon[1]; xin[2] = canon[2];
      }

      st.tl.stamp(3, id);
      float embx[kStepsNerfXyz], ext[kStepsExtraMax];
      if (!(MF_TIMING_FLAGS && (p.dbg & 4))) emb_eval_lds<3, 10>(embx, xin, par_nerf_xyz, id.g);
      else { for (int e = 0; e < kStepsNerfXyz; ++e) embx[e] = xin[e % 3]; }
#pragma unroll
      for (int e = BlkXyz10::SLOTS; e < kStepsNerfXyz; ++e) embx[e] = 0.f;
#pragma unroll
      for (int e = 0; e < kStepsExtraMax; ++e) ext[e] = 0.f;
      float* dump_row = nullptr;
      unsigned* mask_row = nullptr;
      uint32_t ray_bias = 0;                   // FOLD: LDS byte offset of the lane's row of the group's bias table
#if MF_BODY_FOLD
      {
        const Where w = where();
#ifdef MF_RAYBIAS_BREAK_ROW   // (the deliberately broken build tests/test_gpu_ray_bias.py must reject: every lane reads the group's first row)
        const int rr = 0 * (int)(w.ray - ray0);
#else
        const int rr = (int)(w.ray - ray0);
#endif
        ray_bias = p.fold_wx ? p.rbias_off + (uint32_t)rr * (kFoldHalf * 4) : nerf.res_lds + nerf.L.off_bias_extra * 4;
      }
#else
      {
        const Where w = where();
        if (!sigma_only) {
          if (p.extra_type == MF_EXTRA_DIR) {
            const float dd[3] = {w.rp[3], w.rp[4], w.rp[5]};
            emb_eval_lds<3, 4>(ext, dd, par_nerf_ext, id.g);                             // rendering.py:138-142
          } else if (p.extra_type == MF_EXTRA_IND) {
            const float iv[1] = {w.rp[8]};
            emb_eval_lds<1, 2>(ext, iv, par_nerf_ext, id.g);                             // rendering.py:133-137
          }
        }
        if constexpr (DUMP) {
          if (w.valid && p.dump_acts) dump_row = p.dump_acts + (w.ray * S + w.si) * p.dump_stride;
          // (round 4: the chain kernel writes them too -- one more spilled dword in its prologue, two scratch reloads per tile;
          //  the NeRF's dX chain under NoF then reads 32 bytes instead of 1 KiB per layer and sample)
          if (p.dump_mask) mask_row = p.dump_mask + (w.ray * S + w.si) * p.dump_mask_stride;   // (uniformly non-null when asked for)
        }
      }
#endif
      st.tl.stamp(4, id);
      float sigma, rgb[3] = {0.f, 0.f, 0.f};
      st.keep2 = 0;      // the first panel's barrier drains everything (see Stream::sync_and_dma)
      if constexpr (FOLD) nerf_eval<16, DUMP, FOLD, !MOCO>(nerf, embx, ext, sigma_only, st, carry, id, prog_first, sigma, rgb, nullptr, nullptr, ray_bias);
      else
      nerf_eval<16, DUMP, FOLD>(nerf, embx, ext, sigma_only, st, carry, id, prog_first, sigma, rgb, dump_row, mask_row);
      {
        const Where w = where();
        if (w.valid && id.g == 0) {
          sbuf[w.srel] = make_float4(rgb[0], rgb[1], rgb[2], sigma);
          if constexpr (DUMP) {
            const long long row = w.ray * S + w.si;
            if (p.dump_rgbsigma) *reinterpret_cast<float4*>(p.dump_rgbsigma + row * 4) = make_float4(rgb[0], rgb[1], rgb[2], sigma);
            if (p.dump_xyz) { float* q = p.dump_xyz + row * 3; q[0] = xin[0]; q[1] = xin[1]; q[2] = xin[2]; }
          }
        }
      }
      st.tl.stamp(5, id);
    }
    __syncthreads();
    st.tl.stamp(6, id);

    composite_group<kWaves>(p, id.lane, id.wave, ray0, (MF_TIMING_FLAGS && (p.dbg & 8)) ? 0 : nr, S, sigma_only, sbuf, zbuf);
    st.tl.stamp(7, id);
    __syncthreads();
    st.tl.stamp(8, id);
  }
  wait_vm0();   // the stream runs two panels ahead: drain the LDS-DMA before the workgroup retires
  wg.stamp(p);
