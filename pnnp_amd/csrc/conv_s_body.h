// The body of igemm_x3s_kernel<BN, EK> / igemm_h2s_kernel<BN, EK> (csrc/conv_x3s.hip, csrc/conv_h2s.hip): included inside the __global__ wrapper, which supplies
// `Scheme`, BN, EK and the argument `const H2Args ha`.  csrc/conv_s.h says what a Scheme provides and why this is an included text.  (No include guard.)
    static_assert(Scheme::has(EK, BN), "an epilogue the scheme's dispatch does not launch");
    const IgemmArgs& a = ha.g;
    constexpr bool POOL = EK == EK_POOL;
    // element types of the activations (csrc/conv_s.h SElem): fp16 K segments / an fp16 dst[0] and pooled map; LPS: 16-byte loads per staging slot (8 channels)
    constexpr bool SRC16 = SElem<Scheme>::SRC16, DST16 = SElem<Scheme>::DST16;
    constexpr int SRC_ES = SRC16 ? 2 : 4, LPS = SRC16 ? 1 : 2;
    static_assert(!DST16 || EK == EK_FWD || EK == EK_POOL || EK == EK_HEAD || (EK == EK_RES && SRC16), "epilogues with an fp16 destination");
    using Cfg = SCfg<Scheme, BN>;
    constexpr int NT = Cfg::NT, D = Cfg::DPW, XS_F4 = Cfg::XS_F4, XS_BYTES = Cfg::XS_BYTES, NSTAGE = Cfg::NSTAGE, AHEAD = Cfg::AHEAD, ITEMS = Scheme::ITEMS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u32x4* xs = reinterpret_cast<u32x4*>(smem);                     // two halo images
    char* wsb = smem + 2 * XS_BYTES;                                // the weight ring
    float* bias_lds = reinterpret_cast<float*>(smem + 2 * XS_BYTES + NSTAGE * Cfg::WS_STAGE);      // bias[0 .. Ntot) (zeros without a bias)
    float* head_lds = bias_lds + Cfg::BIAS_MAX + 64;                // (EK_HEAD) the head's weights [4][32] and biases [4]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // 0 .. 7 consumers, 8 .. 11 producers

    // ---- scales (scaled schemes, csrc/h2.h): se_x from the largest amax of the K segments, se_w from the weight tensor's
    int se_x = 0, se_w = 0;
    if constexpr (Scheme::SCALED) Scheme::scale_exps(ha, se_x, se_w);

    // ---- the workgroup's tiles t, t + G, ...: decoded once, then stepped by mixed-radix addition (both roles walk the same sequence)
    const int tiles_x = (a.DW + 31) >> 5, tiles_y = (a.DH + TH - 1) / TH;
    const int n_tiles = (a.Ntot + BN - 1) / BN;
    // split-K (general epilogue only; ha.ksplit = S > 1): S workgroups share an output tile, slice ks owning chunks [ks, ks + 1) nchunks / S of K and
    // writing its raw partial sums into image ks B + b of a [S][B][OH][OW][cs] slab tensor; h2_splitk_reduce_kernel adds the slabs in a fixed order
    constexpr bool SPLITK = EK == EK_GEN;
    const int KSPL = SPLITK ? ha.ksplit : 1;
    const int total = tiles_x * tiles_y * a.B * n_tiles * KSPL;
    const int G = gridDim.x;
    const int nchunks = a.nseg * a.chunks_per_seg / KSPL;           // 16-channel chunks of K a workgroup walks per tile (its slice)
    struct Tile { int b, y0, x0, n0, ks; };
    auto decode = [&](int t) {
        Tile o;
        const int nt_i = t % n_tiles;
        int m_i = t / n_tiles;
        const int tx = m_i % tiles_x; m_i /= tiles_x;
        o.x0 = tx * 32; o.y0 = (m_i % tiles_y) * TH; o.b = m_i / tiles_y; o.n0 = nt_i * BN; o.ks = 0;
        if constexpr (SPLITK) { o.ks = o.b / a.B; o.b -= o.ks * a.B; }
        return o;
    };
    auto pick = [](bool c, const Tile& x, const Tile& y) {
        Tile o; o.b = c ? x.b : y.b; o.y0 = c ? x.y0 : y.y0; o.x0 = c ? x.x0 : y.x0; o.n0 = c ? x.n0 : y.n0; o.ks = 0;
        if constexpr (SPLITK) o.ks = c ? x.ks : y.ks;
        return o;
    };
    const Tile gstep = decode(G);
    auto advance = [&](Tile o) {
        o.n0 += gstep.n0; if (o.n0 >= n_tiles * BN) { o.n0 -= n_tiles * BN; o.x0 += 32; }
        o.x0 += gstep.x0; if (o.x0 >= tiles_x * 32) { o.x0 -= tiles_x * 32; o.y0 += TH; }
        o.y0 += gstep.y0; if (o.y0 >= tiles_y * TH) { o.y0 -= tiles_y * TH; o.b += 1; }
        o.b += gstep.b;
        if constexpr (SPLITK) { if (o.b >= a.B) { o.b -= a.B; o.ks += 1; } o.ks += gstep.ks; }
        return o;
    };
    int t = xcd_remap(blockIdx.x, G);
    if (t >= total) return;
    // lookahead of LA tiles: the producers request halo chunks up to max(2, NSETS) chunks ahead, which is that many TILES ahead for a one-chunk layer
    constexpr int NS = Scheme::NSETS, LA = NS > 2 ? NS : 2;
    static_assert(NS >= 1 && NS <= 3, "producer register sets");
    Tile cur = decode(t), ahead[LA];
    ahead[0] = pick(t + G < total, advance(cur), cur);
#pragma unroll
    for (int i = 1; i < LA; ++i) ahead[i] = pick(t + (i + 1) * G < total, advance(ahead[i - 1]), ahead[i - 1]);
    int g = 0;                                                       // chunk of the current tile
    // the k-th chunk after the current one, k = 1 .. LA: (tile, chunk, exists); past the end of this workgroup's work it falls back to the
    // current chunk (requests stay branch-free; weights are then requested with valid = false)
    struct Ck { Tile tile; int g; bool ok; };
    auto chunk_at = [&](auto ktag) {
        constexpr int k = decltype(ktag)::value;
        static_assert(k >= 1 && k <= LA, "lookahead");
        int gk = g + k, hop = 0;
#pragma unroll
        for (int i = 0; i < k; ++i)
            if (gk >= nchunks) { gk -= nchunks; ++hop; }
        Ck c;
        c.ok = t + hop * G < total;
        c.g = c.ok ? gk : g;
        Tile far = ahead[0];
#pragma unroll
        for (int i = 1; i < k; ++i) far = pick(hop > i, ahead[i], far);
        c.tile = pick(!c.ok || hop == 0, cur, far);
        return c;
    };
    auto next_tile = [&]() {
        t += G; cur = ahead[0];
#pragma unroll
        for (int i = 0; i + 1 < LA; ++i) ahead[i] = ahead[i + 1];
        ahead[LA - 1] = pick(t + LA * G < total, advance(ahead[LA - 2]), ahead[LA - 2]);
        g = 0;
    };
    using K1 = std::integral_constant<int, 1>;
    // item number `it` counts work items over the whole run of the workgroup: item `it` lives in stage it % NSTAGE.  The stage k items after stage st:
    auto stage_after = [](int st, int k) { return NSTAGE == 2 ? st ^ (k & 1) : (st + k) % NSTAGE; };

    if (wave >= NCW) {
        // =============================================== PRODUCER ===============================================
        const int pw = wave - NCW, ptid = tid - 64 * NCW;            // 0 .. 3, 0 .. 255
        const float sx = __uint_as_float((unsigned)(se_x + 127) << 23);      // 2^se_x
        // staging slots: s = ptid + 256 k -> (pixel s >> 1, channel octet s & 1); a slot past the end repeats the previous one of the thread
        int rk[NSLOT], qk[NSLOT]; unsigned pixk[NSLOT]; int xdst[NSLOT];
        const int oct = ptid & 1;
#pragma unroll
        for (int k = 0; k < NSLOT; ++k) {
            int s = ptid + PTHR * k;
            if (s >= 2 * NPIX) s -= PTHR;
            const int pix = s >> 1;
            const int r = pix / HC, q = pix - r * HC;
            rk[k] = r - 1; qk[k] = q - 1;
            pixk[k] = (unsigned)(r * a.IW + q);
            xdst[k] = XS_PLANE(0, oct) + pix;                       // + piece * XS_PIECE_STRIDE (+ image * XS_F4)
        }
        const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x7fffffff, 0x00020000);
        f32x4 ra[NS][NSLOT][LPS];                                   // halo chunks in flight / waiting to be split, 8 channels per slot (SRC16: one word, fp16 as loaded)
        // global loads of the halo tile of (tile, chunk gq) -> register set S: hardware zero for pixels outside the image and channels past the segment
        auto load_halo = [&](auto stag, const Tile& tl, int gq) {
            constexpr int S = decltype(stag)::value;
            if constexpr (SPLITK) gq += tl.ks * nchunks;            // (this slice's chunks of K)
            const int si = gq / a.chunks_per_seg, cc = gq - si * a.chunks_per_seg;
            const IgemmSeg sg = a.seg[si];
            const int c0 = sg.coff + cc * 16;
            const int rlo = -tl.y0, rhi = a.IH - tl.y0, qlo = -tl.x0, qhi = a.IW - tl.x0;
            const int shift = (2 * a.IW + 2) * sg.cstride;         // the resource starts before the image: the scalar offset below stays >= 0
            const int64_t first = (int64_t)tl.b * a.IH * a.IW * sg.cstride - shift;      // (elements)
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(SRC16 ? (void*)(reinterpret_cast<const _Float16*>(sg.ptr) + first) : (void*)(sg.ptr + first), 0, 0x7fffffff, 0x00020000);
            const int soff = (((tl.y0 - 1) * a.IW + tl.x0 - 1) * sg.cstride + c0 + shift) * SRC_ES;
            const unsigned cs4 = (unsigned)sg.cstride * (unsigned)SRC_ES;
            const int cvalid = a.seg_channels - cc * 16 - oct * 8;  // > 0: this thread's octet exists
#pragma unroll
            for (int k = 0; k < NSLOT; ++k) {
                const int bad = (rk[k] - rlo) | (rhi - 1 - rk[k]) | (qk[k] - qlo) | (qhi - 1 - qk[k]) | (cvalid - 1);     // sign bit set <=> outside
                const unsigned vo = bad < 0 ? OOB : __umul24(pixk[k], cs4) + oct * (8 * SRC_ES);
                ra[S][k][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, soff, 0));
                if constexpr (!SRC16) ra[S][k][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, soff + 16, 0));
            }
        };
        // the slots of register set S that work item `item` of a chunk splits -> their PIECES 16-byte words (8 channels of each piece) in halo image img
        auto stage = [&](auto stag, auto itag, int img) {
            constexpr int S = decltype(stag)::value, item = decltype(itag)::value;
            constexpr int K0 = item * Scheme::SLOTS, K1 = item + 1 < ITEMS ? K0 + Scheme::SLOTS : NSLOT;
#pragma unroll
            for (int k = K0; k < K1; ++k) {
                if constexpr (SRC16) {                               // the eight halves are the image's word: nothing to split, no scale (se_x = 0)
                    static_assert(!SRC16 || Scheme::PIECES == 1, "an fp16 source is its own single piece");
                    xs[img * XS_F4 + xdst[k]] = __builtin_bit_cast(u32x4, ra[S][k][0]);
                    continue;
                }
                u32x4 sp[Scheme::PIECES];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const f32x4 v = ra[S][k][SRC16 ? 0 : p >> 1];
                    unsigned w[Scheme::PIECES];
                    Scheme::split(v[(p & 1) * 2], v[(p & 1) * 2 + 1], sx, w);
#pragma unroll
                    for (int q = 0; q < Scheme::PIECES; ++q) sp[q][p] = w[q];
                }
                u32x4* d = xs + img * XS_F4 + xdst[k];
#pragma unroll
                for (int q = 0; q < Scheme::PIECES; ++q) d[q * XS_PIECE_STRIDE] = sp[q];
            }
        };
        // LDS-DMA of the weights of item (tile n0, chunk gq, item `row` of the chunk) into stage st: per 32-column block and chunk the pack holds ITEMS x WBLK
        // contiguous bytes, item after item; as 1 KB pieces dealt over the 4 producer waves; past the end a wave repeats the last piece (same bytes, same place)
        const int K16 = a.nseg * a.chunks_per_seg;
        auto dma_weights = [&](const Tile& tl, int gq, auto rowtag, int st, bool valid) {
            constexpr int row = decltype(rowtag)::value;
            if constexpr (SPLITK) gq += tl.ks * nchunks;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const int ins = min(pw + NPW * i, Cfg::NDMA - 1);
                const int j = ins / Cfg::NP1, r = ins - Cfg::NP1 * j;
                const int nb = (tl.n0 >> 5) + j;
                const bool ok = valid && nb * 32 < a.Ntot;        // (an invalid request still issues: the vmcnt counts below count instructions)
                const int soff = ok ? ((nb * K16 + gq) * (ITEMS * Scheme::WBLK) + (row * Cfg::NP1 + r) * 1024) : 0;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (__attribute__((address_space(3))) void*)(wsb + st * Cfg::WS_STAGE + ins * 1024),
                                                         16, ok ? (unsigned)lane * 16u : OOB, soff, 0, 0);
            }
        };
        // Every exact vmcnt wait of the producers.  vmcnt completes in issue order, so "the weights the next barrier releases have landed" is "at most N younger
        // vector-memory instructions are in flight", N = what this wave issued behind those weights:
        //   in front of an item barrier: the next item's weights were requested AHEAD items ago, the weights of the AHEAD - 1 items after them -- (AHEAD - 1) DPW
        //     LDS-DMA instructions -- behind them, and then the 2 NSLOT halo loads of the register set requested behind the weights in THIS item, if it requests
        //     one (halo loads of an earlier item are not counted: the wait covers them too, and their values are split first anyway);
        //   in front of barrier 0: ALL the prologue's weights (items 0 .. AHEAD - 1), behind them the halos of max(1, NSETS - 1) register sets.
        // bf16x3: BN 32 (AHEAD 2, DPW 3) 3, 3, 3 + 10; BN 64 (AHEAD 1) 0, 0, 10; fp16x2 (AHEAD 1, NSETS 2): 10; barrier 0: 10 each.
        auto wait_weights = [](auto items_tag, auto sets_tag) { __builtin_amdgcn_s_waitcnt(CS_VMCNT(decltype(items_tag)::value * D + LPS * NSLOT * decltype(sets_tag)::value)); };
        static_assert((AHEAD - 1) * D + LPS * NSLOT <= 63 && LPS * NSLOT * (NS > 1 ? NS - 1 : 1) <= 63, "the producers' vmcnt");
        // ---- prologue: the bias vector, the padding words of the hi planes where the scheme reads them (fp16x2: the unpaired ninth tap's second half reads
        // one pixel past tap 8: word 612 for the last lane of the last row -- multiplied by the pack's zero tap, so it must be FINITE, not whatever bit pattern
        // the LDS held), the weights of items 0 .. AHEAD - 1, chunk 0's halo straight into image 0, the halos of chunks 1 .. max(1, NS - 1) into the register sets
        for (int i = ptid; i < Cfg::BIAS_MAX + 64; i += PTHR) bias_lds[i] = (a.bias && i < a.Ntot) ? a.bias[i] : 0.f;
        if constexpr (EK == EK_HEAD) {
            if (ptid < 132) head_lds[ptid] = ptid < 128 ? ha.head_w[ptid] : (ha.head_b ? ha.head_b[ptid - 128] : 0.f);
        }
        if constexpr (Scheme::ZERO_PAD) {
            if (ptid < 48) xs[(ptid / 24) * XS_F4 + XS_PLANE(0, (ptid / 12) & 1) + NPIX + ptid % 12] = u32x4{0u, 0u, 0u, 0u};
        }
        // (the requests written out, not a static_for: behind one more lambda the 64-column fp16x2 kernels compiled the requests' range selects as branches)
        dma_weights(cur, 0, std::integral_constant<int, 0>{}, 0, true);
        if constexpr (AHEAD > 1) dma_weights(cur, 0, std::integral_constant<int, 1>{}, 1, true);
        static_assert(AHEAD <= 2, "the prologue's weight requests");
        load_halo(std::integral_constant<int, 0>{}, cur, 0);
        static_for<0, ITEMS>([&](auto rt) { stage(std::integral_constant<int, 0>{}, rt, 0); });
        static_for<1, (NS > 1 ? NS : 2)>([&](auto jt) {             // (past the end: the current chunk again, harmless)
            constexpr int j = decltype(jt)::value;
            const Ck nj = chunk_at(jt);
            load_halo(std::integral_constant<int, j % NS>{}, nj.tile, nj.g);
        });
        wait_weights(std::integral_constant<int, 0>{}, std::integral_constant<int, (NS > 1 ? NS - 1 : 1)>{});      // the weights; the halos stay in flight
        CS_BARRIER();                                             // barrier 0: item 0 may start
        int img = 0, st = 0;                                        // image of the current chunk; stage of its first item
#ifdef CONVS_STAMPS
        long long t_work = 0, t_wait = 0, t_bar = 0, tlast_ = clock64(), tall = tlast_; int nch = 0;
#endif
        // One period = the consumers run chunk c, item by item.  Per item: the weights of item + AHEAD into the stage the consumers left at the last barrier, then
        // a share of the halo work:
        //   NS = 1: the halo of chunk c + 1 (requested at the end of period c - 1) is split into the other image, the item's slots at a time; behind the last
        //           share the registers are free and chunk c + 2's halo is requested;
        //   NS > 1: chunk c + NS's halo is requested FIRST, into the register set chunk c was split out of a period ago, then chunk c + 1's
        //           (set (c + 1) % NS, in flight for NS - 1 whole periods) is split.
        // In front of every barrier the weights of the next item must have landed (wait_weights).  The loop is unrolled NS times (P = c % NS).
        auto period = [&](auto ptag) {
            constexpr int P = decltype(ptag)::value;
            const Ck n1 = chunk_at(K1{}), nl = chunk_at(std::integral_constant<int, (NS > 1 ? NS : 2)>{});
#ifdef CONVS_STAMPS
            ++nch;
#endif
            bool more = true;
            static_for<0, ITEMS>([&](auto rt) {
                constexpr int r = decltype(rt)::value;
                constexpr bool LOADS = NS == 1 ? r == ITEMS - 1 : r == 0;      // this item requests a halo
                // the weights of the item AHEAD items on (AHEAD <= ITEMS: an item of this chunk or of the next)
                if constexpr (r + AHEAD < ITEMS) dma_weights(cur, g, std::integral_constant<int, r + AHEAD>{}, stage_after(st, r + AHEAD), true);
                else dma_weights(n1.tile, n1.g, std::integral_constant<int, r + AHEAD - ITEMS>{}, stage_after(st, r + AHEAD), n1.ok);
                if constexpr (NS == 1) {
                    stage(std::integral_constant<int, 0>{}, rt, img ^ 1);
                    if constexpr (LOADS) load_halo(std::integral_constant<int, 0>{}, nl.tile, nl.g);
                } else {
                    if constexpr (LOADS) load_halo(ptag, nl.tile, nl.g);
                    stage(std::integral_constant<int, (P + 1) % NS>{}, rt, img ^ 1);
                }
                CS_T(t_work)
                wait_weights(std::integral_constant<int, AHEAD - 1>{}, std::integral_constant<int, LOADS ? 1 : 0>{});
                CS_T(t_wait)
                if constexpr (r == ITEMS - 1) { if (!n1.ok) { more = false; return; } }      // (the consumers' epilogue and exit need no barrier)
                CS_BARRIER();
                CS_T(t_bar)
            });
            if (!more) return false;
            if (g == nchunks - 1) next_tile(); else ++g;
            img ^= 1; st = stage_after(st, ITEMS);
            return true;
        };
        for (;;) {
            if (!period(std::integral_constant<int, 0>{})) break;
            if constexpr (NS > 1) { if (!period(std::integral_constant<int, 1>{})) break; }
            if constexpr (NS > 2) { if (!period(std::integral_constant<int, 2>{})) break; }
        }
#ifdef CONVS_STAMPS
        if (lane == 0) {
            float* d = a.dst[0] + ((int64_t)blockIdx.x * (NCW + NPW) + wave) * 8;
            d[0] = (float)t_work; d[1] = (float)t_wait; d[2] = (float)t_bar; d[3] = 0.f; d[4] = (float)(clock64() - tall); d[5] = (float)nch;
        }
#endif
        return;
    }

    // =============================================== CONSUMER ===============================================
    // 16 x 16 accumulator blocks, WEIGHTS as the instruction's first operand: acc[2 i + h][j] = pixel row i of the wave, 16-pixel half h,
    // channels 16 j .. 16 j + 15; lane l holds channels 4 (l >> 4) .. + 3 of pixel l & 15
    constexpr int MB = 2 * MT, NB = BN / 16;
    f32x4 acc[MB][NB];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- the epilogue's kernel arguments, cached in ONE vector register (lane i = argument i) and fetched with v_readlane: the unrolled K loop
    // leaves the compiler no scalar registers for them, and it then RE-LOADS each from the kernel-argument segment where the epilogue uses it
    // (s_load + s_waitcnt lgkmcnt(0), 200-300 cycles a piece, ~25 per tile: cycle stamps of the first version put a forward epilogue at 9000
    // cycles per tile).  The layer's bias vector sits in LDS (written once by the producers) for the same reason: no memory latency here.
    enum { E_OH, E_OW, E_DH, E_DW, E_NTOT, E_NSPLIT, E_ACT, E_POOLCS, E_CS0, E_CS1, E_MM0, E_MM1, E_AC0, E_AC1, E_DEXP, E_NBLK0, E_NBLK1,
           E_DST0, E_DST1 = E_DST0 + 2, E_MASK0 = E_DST1 + 2, E_MASK1 = E_MASK0 + 2, E_ADD = E_MASK1 + 2, E_PDST = E_ADD + 2,
           E_PCODE = E_PDST + 2, E_BOUT = E_PCODE + 2, E_BIN0 = E_BOUT + 2, E_BIN1 = E_BIN0 + 2, E_HOUT = E_BIN1 + 2, E_HRES = E_HOUT + 2, E_COUNT = E_HRES + 2 };
    static_assert(E_COUNT <= 64, "one lane per cached argument");
    unsigned argv = 0;
    {
        auto put = [&](int idx, unsigned v) { argv = lane == idx ? v : argv; };
        auto putp = [&](int idx, const void* q) { put(idx, (unsigned)(uintptr_t)q); put(idx + 1, (unsigned)((uintptr_t)q >> 32)); };
        put(E_OH, a.OH); put(E_OW, a.OW); put(E_DH, a.DH); put(E_DW, a.DW); put(E_NTOT, a.Ntot); put(E_NSPLIT, a.n_split); put(E_ACT, a.act);
        put(E_POOLCS, a.pool_cs); put(E_CS0, a.dst_cs[0]); put(E_CS1, a.dst_cs[1]); put(E_MM0, a.mask_mode[0]); put(E_MM1, a.mask_mode[1]);
        put(E_AC0, a.accum[0]); put(E_AC1, a.accum[1]); put(E_DEXP, (unsigned)(-(se_x + se_w))); put(E_NBLK0, ha.bits_nblk[0]); put(E_NBLK1, ha.bits_nblk[1]);
        putp(E_DST0, a.dst[0]); putp(E_DST1, a.dst[1]); putp(E_MASK0, a.mask[0]); putp(E_MASK1, a.mask[1]); putp(E_ADD, a.addsrc);
        if constexpr (EK == EK_BWDU) { putp(E_PDST, ha.unpool_g); putp(E_PCODE, ha.unpool_codes); }
        else { putp(E_PDST, a.pool_dst); putp(E_PCODE, a.pool_codes); }
        putp(E_BOUT, ha.bits_out); putp(E_BIN0, ha.bits_in[0]); putp(E_BIN1, ha.bits_in[1]);
        putp(E_HOUT, ha.head_out); putp(E_HRES, ha.head_res);
    }
    struct EpiArgs {
        int OH, OW, DH, DW, Ntot, n_split, act, pool_cs, cs0, cs1, mm0, mm1, ac0, ac1, dexp, nblk0, nblk1;
        float *dst0, *dst1, *pool_dst; const float *mask0, *mask1, *addsrc; unsigned char* pool_codes;
        const float* unpool_g; const unsigned char* unpool_codes;      // (EK_BWDU) the pooled map's gradient and the forward pass's codes: inputs
        unsigned* bits_out; const unsigned *bin0, *bin1;
        float* head_out; const float* head_res;
        __device__ int dst_cs(int du) const { return du ? cs1 : cs0; }
        __device__ int mask_mode(int du) const { return du ? mm1 : mm0; }
        __device__ int accum(int du) const { return du ? ac1 : ac0; }
        __device__ float* dst(int du) const { return du ? dst1 : dst0; }
        __device__ const float* mask(int du) const { return du ? mask1 : mask0; }
        __device__ const unsigned* bits_in(int du) const { return du ? bin1 : bin0; }
        __device__ int nblk(int du) const { return du ? nblk1 : nblk0; }
    };
    auto epi_args = [&]() {
        auto rl = [&](int idx) { return (int)__builtin_amdgcn_readlane((int)argv, idx); };
        auto rp = [&](int idx) { return (uintptr_t)(unsigned)rl(idx) | ((uintptr_t)(unsigned)rl(idx + 1) << 32); };
        EpiArgs e;
        e.OH = rl(E_OH); e.OW = rl(E_OW); e.DH = rl(E_DH); e.DW = rl(E_DW); e.Ntot = rl(E_NTOT); e.n_split = rl(E_NSPLIT); e.act = rl(E_ACT);
        e.pool_cs = rl(E_POOLCS); e.cs0 = rl(E_CS0); e.cs1 = rl(E_CS1); e.mm0 = rl(E_MM0); e.mm1 = rl(E_MM1); e.ac0 = rl(E_AC0); e.ac1 = rl(E_AC1);
        e.dexp = rl(E_DEXP); e.nblk0 = rl(E_NBLK0); e.nblk1 = rl(E_NBLK1);
        e.dst0 = (float*)rp(E_DST0); e.dst1 = (float*)rp(E_DST1); e.mask0 = (const float*)rp(E_MASK0); e.mask1 = (const float*)rp(E_MASK1);
        e.addsrc = (const float*)rp(E_ADD);
        if constexpr (EK == EK_BWDU) { e.unpool_g = (const float*)rp(E_PDST); e.unpool_codes = (const unsigned char*)rp(E_PCODE); e.pool_dst = nullptr; e.pool_codes = nullptr; }
        else { e.pool_dst = (float*)rp(E_PDST); e.pool_codes = (unsigned char*)rp(E_PCODE); e.unpool_g = nullptr; e.unpool_codes = nullptr; }
        e.bits_out = (unsigned*)rp(E_BOUT); e.bin0 = (const unsigned*)rp(E_BIN0); e.bin1 = (const unsigned*)rp(E_BIN1);
        if constexpr (EK == EK_HEAD) { e.head_out = (float*)rp(E_HOUT); e.head_res = (const float*)rp(E_HRES); }
        return e;
    };
    float amx0 = 0.f, amx1 = 0.f;                                    // (SCALED) max |stored value| of this lane, per destination
    f32x4 hw[EK == EK_HEAD ? 8 : 1];                                 // (EK_HEAD) head weights of this lane's 8 channels: [output o][16-column block jj] (loaded behind barrier 0)

    // (EK_BWDB) the tile's mask words, requested in FRONT of its last chunk (round 6): requested at the start of the epilogue, the first
    // mask_scale waited a memory latency for them with the matrix pipe idle -- per tile, ~2 000 cycles of a 13 000 ... 40 000-cycle tile on the shallow layers
    unsigned mbits_pre[(EK == EK_BWDB || EK == EK_BWDU) ? NT : 1];
    auto prefetch_bits = [&](const Tile& tl) __attribute__((always_inline)) {
        const EpiArgs ea = epi_args();
        int lane_p = lane;
        asm volatile("" : "+v"(lane_p));
        const int tile_id = (tl.b * tiles_y + tl.y0 / TH) * tiles_x + (tl.x0 >> 5);
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const int nwv = __builtin_amdgcn_readfirstlane(tl.n0 + k * 32);
            const int du = nwv >= ea.n_split ? 1 : 0, chw = nwv - (du ? ea.n_split : 0), nblk = ea.nblk(du);
            const unsigned* bp = ea.bits_in(du);
            const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(bp ? bp : ea.bin0), 0, a.B * tiles_y * tiles_x * nblk * NCW * 64 * 4, 0x00020000);
            const unsigned off = (unsigned)((((tile_id * nblk + (chw >> 5)) * NCW + wave) * 64 + lane_p) * 4);
            mbits_pre[k] = __builtin_amdgcn_raw_buffer_load_b32(rb, (ea.mask_mode(du) && bp && nwv < ea.Ntot) ? off : OOB, 0, 0);
        }
    };

    // (EK_BWDU) the pooled gradient and the codes behind this lane's store addresses: [32-column block k][16-pixel half h][store instruction 1 / 2], requested in
    // front of the tile's last chunk too.  Instruction 1
    // of (k, i, h) writes pixel (y0 + 2 w + i, x0 + (l & 7) + 16 h), channels 32 k + (l & 8 ? 16 : 0) + 4 (l >> 4) .. + 3, instruction 2 the pixel 8 on: pooled
    // pixel ((y0 >> 1) + w, (x >> 1)) for both rows i -- the `po` of the EK_POOL forward epilogue, read.  Outside the map / the tensor: out of range, zeros.
    constexpr int NPG = EK == EK_BWDU ? NT : 1;
    f32x4 pg_pre[NPG][2][2]; unsigned pc_pre[NPG][2][2];
    auto prefetch_pool = [&](const Tile& tl) __attribute__((always_inline)) {
        const EpiArgs ea = epi_args();
        int lane_p = lane;
        asm volatile("" : "+v"(lane_p));
        const int ph = ea.OH >> 1, pwd = ea.OW >> 1;
        const int64_t pimg = (int64_t)tl.b * ph * pwd * ea.pool_cs;
        const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)(ea.unpool_g + pimg), 0, ph * pwd * ea.pool_cs * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void*)(ea.unpool_codes + pimg), 0, ph * pwd * ea.pool_cs, 0x00020000);
        const int y = tl.y0 + wave * MT, xl = tl.x0 + (lane_p & 7);
        const int chl = ((lane_p & 8) ? 16 : 0) + (lane_p >> 4) * 4;
#pragma unroll
        for (int k = 0; k < NPG; ++k) {
            const int nwv = __builtin_amdgcn_readfirstlane(tl.n0 + k * 32);
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const int x = xl + 16 * h + 8 * s2;
                    const bool ok = nwv < ea.Ntot && y < ea.DH && x < ea.DW;
                    const unsigned po = (unsigned)(((y >> 1) * pwd + (x >> 1)) * ea.pool_cs + nwv + chl);
                    pg_pre[k][h][s2] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rp, ok ? po * 4u : OOB, 0, 0));
                    pc_pre[k][h][s2] = __builtin_amdgcn_raw_buffer_load_b32(rc, ok ? po : OOB, 0, 0);
                }
        }
    };

    // ---- epilogue of tile `tl`, straight from the accumulators: x 2^dexp (undo the operand scales), bias, activation, act' mask, residual and
    // accumulation are float4 arithmetic on the accumulator registers.  The fused
    // MaxPool2d(2) takes the other pixel of a pair from the neighbouring lane (DPP) and the other row from the wave's second accumulator row.
    auto epilogue = [&](const Tile& tl) __attribute__((always_inline)) {
        const EpiArgs ea = epi_args();
        const int b = SPLITK ? tl.b + tl.ks * a.B : tl.b, n0 = tl.n0;     // (split-K: slab image ks B + b; the launcher allows no mask / residual / bits there)
        // the lane number as an OPAQUE value: everything the epilogue derives from it is then computed here, per tile (a dozen instructions),
        // instead of being hoisted in front of the K loop and carried through it in ~50 registers (19 of them spilled to scratch in the
        // 64-column forward kernel: cycle stamps 14 600 cycles per forward tile against 10 000 for the spill-free backward-data kernel)
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));
        const int p16 = lane_e & 15, c4 = (lane_e >> 4) * 4;
        const int py0 = tl.y0 + wave * MT, px0 = tl.x0 + p16;
        int du_[NT], chw_[NT], cs_[NT]; bool blk_[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const int nwv = __builtin_amdgcn_readfirstlane(n0 + k * 32);
            du_[k] = nwv >= ea.n_split ? 1 : 0; chw_[k] = nwv - (du_[k] ? ea.n_split : 0); cs_[k] = ea.dst_cs(du_[k]); blk_[k] = nwv < ea.Ntot;
        }
        // is this lane's own pixel (row i, 16-pixel half h) inside the map?  (lane masks: scalar registers)
        bool okp[MT][2];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) okp[i][h] = py0 + i < ea.DH && px0 + 16 * h < ea.DW;
        // (general epilogue) byte offset of that pixel and the lane's channel quad in the destination of 32-column block k, or out of range;
        // the 16-column block inside it (+ 64 bytes) goes through the instruction's scalar offset
        unsigned vo[EK == EK_GEN ? NT : 1][MT][2];
        if constexpr (EK == EK_GEN) {
#pragma unroll
            for (int k = 0; k < NT; ++k)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        vo[k][i][h] = (blk_[k] && okp[i][h]) ? (unsigned)((((py0 + i) * ea.OW + px0 + 16 * h) * cs_[k] + chw_[k] + c4) * 4) : OOB;
        }
        auto rsrc = [&](const float* base, int k) {
            return __builtin_amdgcn_make_buffer_rsrc((void*)(base + (int64_t)b * ea.OH * ea.OW * cs_[k]), 0, ea.OH * ea.OW * cs_[k] * 4, 0x00020000);
        };
        // this lane's word of the tile-private bit layout (csrc/h2.h) for 32-column block k of a tensor with nblk channel blocks, in bytes
        const int tile_id = (b * tiles_y + tl.y0 / TH) * tiles_x + (tl.x0 >> 5);
        auto bits_off = [&](int k, int nblk) { return (unsigned)((((tile_id * nblk + (chw_[k] >> 5)) * NCW + wave) * 64 + lane_e) * 4); };
        auto bits_rsrc = [&](const unsigned* base, int nblk) {
            return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, a.B * tiles_y * tiles_x * nblk * NCW * 64 * 4, 0x00020000);
        };
        const float aslope = ea.act == 1 ? 0.2f : (ea.act == 2 ? 0.f : 1.f);
        f32x4 bias4[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            bias4[j] = *reinterpret_cast<const f32x4*>(bias_lds + n0 + 16 * j + c4);      // (columns past Ntot: zeros, and their stores are dropped anyway)
        }
        auto act4 = [&](f32x4 o) {                                   // LeakyReLU(0.2) / ReLU / none as max(o, slope * o)
            const f32x4 t = o * aslope;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = fmaxf(o[c], t[c]);
            return o;
        };
        // (SCALED) Undoing the operand scales: x 2^dexp (exact).  As ONE multiplier (fused with the bias add where there is one) while 2^dexp is a normal
        // float32 with room for the LeakyReLU slope; tensors so small / large that it is not (|dexp| > 120: max |x| max |w| beyond 2^+-92) first take the remainder in a pass over the
        // accumulators -- a wave-uniform branch that the networks' tensors never take (tests/test_gpu_h2.py::test_h2_dynamic_range does).
        const int dexp_c = ea.dexp < -120 ? -120 : (ea.dexp > 120 ? 120 : ea.dexp);      // (|.| <= 120: 0.2 x 2^dexp_c stays a normal float32, see mask_scale)
        const float dsc = __uint_as_float((unsigned)(dexp_c + 127) << 23);
        if constexpr (Scheme::SCALED) {
            if (ea.dexp != dexp_c) {
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int j = 0; j < NB; ++j)
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[mb][j][c] = __builtin_ldexpf(acc[mb][j][c], ea.dexp - dexp_c);
            }
        }
        auto take_raw = [&](int mb, int j) {                         // the accumulator block as it is (the caller scales), zeroed for the next tile
            const f32x4 v = acc[mb][j];
            acc[mb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            return v;
        };
        auto take = [&](int mb, int j) {                             // the block, un-scaled
            const f32x4 v = take_raw(mb, j);
            if constexpr (Scheme::SCALED) return v * dsc; else return v;
        };
        auto take_bias = [&](int mb, int j, f32x4 bias) {            // ... with the bias: one fma per element
            const f32x4 v = take_raw(mb, j);
            if constexpr (Scheme::SCALED) return f32x4{__builtin_fmaf(v.x, dsc, bias.x), __builtin_fmaf(v.y, dsc, bias.y), __builtin_fmaf(v.z, dsc, bias.z), __builtin_fmaf(v.w, dsc, bias.w)};
            else return v + bias;
        };
        // (SCALED) max |.| of the blocks of one destination: a running maximum per 32-column block (two v_max3_f32 per float4), merged into the lane's
        // maximum of that destination once per block.  Lanes whose store is dropped (pixels / columns outside the tensor) count too: what
        // they hold are finite sums over zero padding, and an amax slot may over-estimate (csrc/h2.h) -- masking them was a compare and
        // two selects per float4.
        float amk = 0.f;
        auto track = [&](f32x4 o) {
            if constexpr (!Scheme::SCALED) return;
            amk = fmaxf(fmaxf(amk, fabsf(o.x)), fabsf(o.y));
            amk = fmaxf(fmaxf(amk, fabsf(o.z)), fabsf(o.w));
        };
        auto track_done = [&](int du) {
            if constexpr (!Scheme::SCALED) return;
            if (du) amx1 = fmaxf(amx1, amk); else amx0 = fmaxf(amx0, amk);
            amk = 0.f;
        };
        // (BITS) Sign bits: element n = ((i 2 + h) 2 + jj) 4 + c of a 32-column block sits at bit 31 - n of the lane's word -- the order in which the
        // forward epilogue produces the values, so that it can SHIFT them in (sb = 2 sb + (o > 0): a compare and an add-with-carry per element) and
        // the backward epilogue can shift them out (carry of sb + sb).  signs4: the generic form (pool and tests).
        auto signs4 = [&](f32x4 o, int pos) {
            return ((o.x > 0.f ? 8u : 0u) | (o.y > 0.f ? 4u : 0u) | (o.z > 0.f ? 2u : 0u) | (o.w > 0.f ? 1u : 0u)) << (28 - pos);
        };
        // one element of the forward epilogue: shift (o > 0) into sb; with an activation o = (o > 0) ? o : slope o on the same compare.  Without sign bits:
        // the activation as max(o, slope o)
        auto act_sign = [](float& o, unsigned& sb, float slope_, auto act_tag) __attribute__((always_inline)) {
            if constexpr (!Scheme::BITS) { if constexpr (decltype(act_tag)::value) o = fmaxf(o, o * slope_); return; }
            unsigned long long cout_;
            if constexpr (decltype(act_tag)::value) {
                float t;
                asm("v_cmp_lt_f32 vcc, 0, %0\n\tv_addc_co_u32 %1, %2, %1, %1, vcc\n\tv_mul_f32 %3, %4, %0\n\tv_cndmask_b32 %0, %3, %0, vcc"
                    : "+v"(o), "+v"(sb), "=s"(cout_), "=&v"(t) : "v"(slope_) : "vcc");
            } else {
                asm("v_cmp_lt_f32 vcc, 0, %2\n\tv_addc_co_u32 %0, %1, %0, %0, vcc" : "+v"(sb), "=s"(cout_) : "v"(o) : "vcc");
            }
        };
        // one element of the bit-masked backward epilogue, scale included: the next bit of mb out (carry of mb + mb), o = v x (bit ? 2^dexp : msl 2^dexp) --
        // three instructions where scaling first and masking afterwards took four; bit-identical: 2^dexp is a power of two, so (v 2^dexp) msl == v (2^dexp msl)
        auto mask_scale = [](float v, unsigned& mb_, float fpos, float fneg) __attribute__((always_inline)) {
            float f, o;
            asm("v_add_co_u32 %2, vcc, %2, %2\n\tv_cndmask_b32 %1, %4, %3, vcc\n\tv_mul_f32 %0, %1, %5" : "=v"(o), "=&v"(f), "+v"(mb_) : "v"(fpos), "v"(fneg), "v"(v) : "vcc");
            return o;
        };
        // ---- FULL-LINE memory pattern (every epilogue but the general one).  Straight from the accumulators a 16-byte store instruction covers 16 pixels x
        // 64 bytes -- sixteen half lines -- and a CU then stores 21 bytes per cycle where 8 pixels x 128 bytes run at 63 and 1 KB contiguous at 84
        // (tools/ubench/store_rate.hip, profiles/r4/store_rate.txt): 6000 of a 64-column tile's cycles.  So the two 16-column blocks of a 32-column block
        // trade halves first: lanes p < 8 of a 16-lane row send the UPPER block of their pixel to lane p + 8 and get the LOWER block of pixel p + 8 back (one
        // DPP row rotation by 8).  Instruction 1 then writes pixels 0-7 (lanes p < 8: their own lower quads, lanes p >= 8: the upper quads of pixel p - 8),
        // instruction 2 pixels 8-15: eight whole 128-byte lines each.  The float32 act' masks come in by the same pattern and are traded back.
        const bool lo8 = p16 < 8;
        auto ror8 = [&](f32x4 v) {                               // (inline assembly: see the pool path about __builtin_amdgcn_update_dpp)
            float r0, r1, r2, r3;
            asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %4 row_ror:8 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %1, %5 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
                         "v_mov_b32_dpp %2, %6 row_ror:8 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %3, %7 row_ror:8 row_mask:0xf bank_mask:0xf"
                         : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3) : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
            return f32x4{r0, r1, r2, r3};
        };
        auto sel = [&](bool c, f32x4 x, f32x4 y) { return f32x4{c ? x.x : y.x, c ? x.y : y.y, c ? x.z : y.z, c ? x.w : y.w}; };
        // The trade of the two 16-column blocks of a pair IN PLACE: afterwards o0 is what store instruction 1 writes (lanes p < 8: their own lower
        // quad, lanes p >= 8: the upper quad of pixel p - 8) and o1 what instruction 2 writes.  A DPP row rotation by 8 whose bank mask enables
        // only the receiving half of each 16-lane row: two moves per register pair + one copy (the select-rotate-select form took four + four).
        auto trade = [&](f32x4& o0, f32x4& o1) __attribute__((always_inline)) {
            float a0 = o0.x, a1 = o0.y, a2 = o0.z, a3 = o0.w, b0 = o1.x, b1 = o1.y, b2 = o1.z, b3 = o1.w;
            const float t0 = b0, t1 = b1, t2 = b2, t3 = b3;
            asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %4 row_ror:8 row_mask:0xf bank_mask:0x3\n\tv_mov_b32_dpp %1, %5 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
                         "v_mov_b32_dpp %2, %6 row_ror:8 row_mask:0xf bank_mask:0x3\n\tv_mov_b32_dpp %3, %7 row_ror:8 row_mask:0xf bank_mask:0x3"
                         : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3) : "v"(a0), "v"(a1), "v"(a2), "v"(a3));
            asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %4 row_ror:8 row_mask:0xf bank_mask:0xc\n\tv_mov_b32_dpp %1, %5 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
                         "v_mov_b32_dpp %2, %6 row_ror:8 row_mask:0xf bank_mask:0xc\n\tv_mov_b32_dpp %3, %7 row_ror:8 row_mask:0xf bank_mask:0xc"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(t0), "v"(t1), "v"(t2), "v"(t3));
            o0 = f32x4{a0, a1, a2, a3}; o1 = f32x4{b0, b1, b2, b3};
        };
        // this lane's byte offset in instruction 1 of block k: pixel (row i, half h, p16 & 7), quad q16 of the lower / upper 16 columns
        unsigned wo[NT][MT][2];
        const int pxl = tl.x0 + (p16 & 7);
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const bool ok = blk_[k] && py0 + i < ea.DH && pxl + 16 * h < ea.DW;
                    wo[k][i][h] = ok ? (unsigned)((((py0 + i) * ea.OW + pxl + 16 * h) * cs_[k] + chw_[k] + (lo8 ? 0 : 16) + c4) * 4) : OOB;
                }
        auto wo2 = [&](int k, int i, int h) {                    // instruction 2: eight pixels on
            return (wo[k][i][h] != OOB && pxl + 16 * h + 8 < ea.DW) ? wo[k][i][h] + (unsigned)(8 * cs_[k] * 4) : OOB;
        };
        // ---- (DST16) the same stores with 2-byte channels.  A pixel's 32 channels are 64 bytes, a lane's two quads 8 bytes each: the four lanes of a pixel
        // (16-lane rows q = 0 .. 3 of the wave) first swap quads so that each holds 8 CONSECUTIVE channels -- v_permlane16_swap: the odd rows of the lower block's
        // packed quad against the even rows of the upper block's; row q then holds channels 16 (q & 1) + 8 (q >> 1) .. + 7 of its pixel -- and ONE 16-byte store
        // instruction writes 16 pixels x 64 bytes: 1 KB contiguous where the channel stride is 32, sixteen half lines where it is wider.  The conversion is
        // one round to nearest even (v_cvt_pk_f16_f32: subnormals kept, no saturation, NaN stays NaN).
        auto pack16 = [&](f32x4 o0, f32x4 o1) __attribute__((always_inline)) {
            typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
            unsigned a0 = __builtin_bit_cast(unsigned, f16x2{(_Float16)o0.x, (_Float16)o0.y}), a1 = __builtin_bit_cast(unsigned, f16x2{(_Float16)o0.z, (_Float16)o0.w});
            unsigned b0 = __builtin_bit_cast(unsigned, f16x2{(_Float16)o1.x, (_Float16)o1.y}), b1 = __builtin_bit_cast(unsigned, f16x2{(_Float16)o1.z, (_Float16)o1.w});
            const auto s0 = __builtin_amdgcn_permlane16_swap(a0, b0, false, false), s1 = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);
            return u32x4{s0[0], s1[0], s0[1], s1[1]};
        };
        const int ch16 = ((lane_e >> 4) & 1) * 16 + (lane_e >> 5) * 8;      // first channel (inside a 32-column block) of the lane's word behind the swap
        unsigned wo16[DST16 ? NT : 1][MT][2];
        if constexpr (DST16) {
#pragma unroll
            for (int k = 0; k < NT; ++k)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        wo16[k][i][h] = (blk_[k] && okp[i][h]) ? (unsigned)((((py0 + i) * ea.OW + px0 + 16 * h) * cs_[k] + chw_[k] + ch16) * 2) : OOB;
        }
        auto rsrc16 = [&](const float* base, int k) {
            return __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<const _Float16*>(base) + (int64_t)b * ea.OH * ea.OW * cs_[k]), 0, ea.OH * ea.OW * cs_[k] * 2, 0x00020000);
        };
        if constexpr (POOL) {
            // Forward layer in front of MaxPool2d(2) (archs/Unet.py:35,41,47,53): single destination, bias + activation only.  A wave owns rows
            // 2w, 2w + 1 of its 32 columns: a lane's two accumulator rows + the same two of lane ^ 1 are one 2x2 window of 4 channels; the even
            // lane writes the pooled float4 and the four codes (bits 0-1 first maximum in the order (0,0) (0,1) (1,0) (1,1), bits 2-5 the signs)
            // of csrc/misc.hip maxpool_fwd_codes_kernel.
            static_assert(MT == 2, "a wave owns one row pair");
            const __amdgpu_buffer_rsrc_t rd = DST16 ? rsrc16(ea.dst(0), 0) : rsrc(ea.dst(0), 0);
            const __amdgpu_buffer_rsrc_t rb = bits_rsrc(ea.bits_out, ea.nblk0);
            const int ph = ea.OH >> 1, pwd = ea.OW >> 1;
            const int64_t pimg = (int64_t)b * ph * pwd * ea.pool_cs;
            const __amdgpu_buffer_rsrc_t rp = DST16 ? __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<_Float16*>(ea.pool_dst) + pimg), 0, ph * pwd * ea.pool_cs * 2, 0x00020000)
                                                    : __builtin_amdgcn_make_buffer_rsrc((void*)(ea.pool_dst + pimg), 0, ph * pwd * ea.pool_cs * 4, 0x00020000);
            const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void*)(ea.pool_codes + pimg), 0, ph * pwd * ea.pool_cs, 0x00020000);
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                unsigned sb = 0u;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    f32x4 wn[2][2];                                  // [16-column block of the pair][row]
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            wn[jj][i] = act4(take_bias(2 * i + h, 2 * k + jj, bias4[2 * k + jj]));      // (SCALED: one fma for scale + bias: bit-identical, v 2^dexp is exact)
                            track(wn[jj][i]);
                            if constexpr (Scheme::BITS) sb |= signs4(wn[jj][i], ((i * 2 + h) * 2 + jj) * 4);
                        }
#pragma unroll
                    for (int i = 0; i < 2; ++i) {                     // full resolution: whole lines (the halves of the block pair traded)
                        if constexpr (DST16) {
                            __builtin_amdgcn_raw_buffer_store_b128(pack16(wn[0][i], wn[1][i]), rd, wo16[k][i][h], 0, CONVS_STORE_AUX);
                            continue;
                        }
                        const f32x4 ox = ror8(sel(lo8, wn[1][i], wn[0][i]));
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, sel(lo8, wn[0][i], ox)), rd, wo[k][i][h], 0, CONVS_STORE_AUX);
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, sel(lo8, ox, wn[1][i])), rd, wo2(k, i, h), 0, CONVS_STORE_AUX);
                    }
                    f32x4 mx16[DST16 ? 2 : 1];                        // (DST16) the pooled quads of both 16-column blocks: one swapped word per lane
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        const int j = 2 * k + jj;
                        const f32x4 (&win)[2] = wn[jj];
                        f32x4 nbr[2];
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            // the pixel to the right (even lanes) / left (odd lanes): quad_perm [1, 0, 3, 2].  As inline assembly (with the two wait
                            // states a DPP read needs behind the VALU write of its source): through __builtin_amdgcn_update_dpp the compiler's DPP
                            // combiner folded the four moves of a float4 into consumers reading element 0 (ROCm 7.2, caught by the pool parity test)
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                float nv; const float sv = win[i][c];
                                asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=v"(nv) : "v"(sv));
                                nbr[i][c] = nv;
                            }
                        }
                        f32x4 mx;
                        unsigned code = 0;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const float w0 = win[0][c], w1 = nbr[0][c], w2 = win[1][c], w3 = nbr[1][c];
                            unsigned arg = 0; float best = w0;
                            if (w1 > best) { best = w1; arg = 1; }                  // first maximum wins
                            if (w2 > best) { best = w2; arg = 2; }
                            if (w3 > best) { best = w3; arg = 3; }
                            const unsigned cj = arg | (w0 > 0.f ? 4u : 0u) | (w1 > 0.f ? 8u : 0u) | (w2 > 0.f ? 16u : 0u) | (w3 > 0.f ? 32u : 0u);
                            mx[c] = fmaxf(fmaxf(w0, w1), fmaxf(w2, w3));
                            code |= cj << (8 * c);
                        }
                        const int px = px0 + 16 * h;
                        const bool ok2 = !(lane_e & 1) && blk_[k] && py0 < ea.DH && px < ea.DW;      // even sizes: the whole window is inside or outside
                        const unsigned po = (unsigned)(((py0 >> 1) * pwd + (px >> 1)) * ea.pool_cs + n0 + 16 * j + c4);
                        if constexpr (DST16) mx16[jj] = mx;
                        else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, mx), rp, ok2 ? po * 4u : OOB, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b32(code, rc, ok2 ? po : OOB, 0, 0);
                    }
                    if constexpr (DST16) {
                        const int px = px0 + 16 * h;
                        const bool ok2 = !(lane_e & 1) && blk_[k] && py0 < ea.DH && px < ea.DW;
                        const unsigned po = (unsigned)(((py0 >> 1) * pwd + (px >> 1)) * ea.pool_cs + n0 + 32 * k + ch16);
                        __builtin_amdgcn_raw_buffer_store_b128(pack16(mx16[0], mx16[1]), rp, ok2 ? po * 2u : OOB, 0, 0);
                    }
                }
                if constexpr (Scheme::BITS) __builtin_amdgcn_raw_buffer_store_b32(sb, rb, (ea.bits_out && blk_[k]) ? bits_off(k, ea.nblk0) : OOB, 0, 0);
                track_done(0);
            }
            return;
        }
        // ---- FWD: no mask, no accumulation, no residual (every forward layer; sign bits on request);  BWD / BWDB: act' masks as float32
        // activations / as the forward kernel's bits (a destination without one requests them out of range: zeros come back, no memory traffic).
        if constexpr (EK == EK_FWD || EK == EK_BWD || EK == EK_BWDB || EK == EK_HEAD || EK == EK_RES || EK == EK_BWDU) {
            constexpr bool RES = EK == EK_RES, UNP = EK == EK_BWDU;
            constexpr bool MASKED = EK == EK_BWD, BITS = EK == EK_BWDB || UNP, FWDL = EK == EK_FWD || EK == EK_HEAD;
            constexpr bool RES16 = RES && DST16;                  // an fp16 residual beside the fp16 destination: one 16-byte word per store instruction
            f32x4 mk[((MASKED || RES) && !RES16) ? MB : 1][((MASKED || RES) && !RES16) ? NB : 1];      // [.][2 k] = what instruction 1 fetched, [.][2 k + 1] = instruction 2 (EK_RES: the residual words)
            u32x4 mk16[RES16 ? MB : 1][RES16 ? NT : 1];            // (RES16) the residual's eight halves at the store's own offset: the post-swap arrangement of pack16
            unsigned mbits[NT];
            if constexpr (RES16) {
#pragma unroll
                for (int k = 0; k < NT; ++k) {
                    const __amdgpu_buffer_rsrc_t rm = rsrc16(ea.addsrc, k);
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int h = 0; h < 2; ++h) mk16[2 * i + h][k] = __builtin_amdgcn_raw_buffer_load_b128(rm, wo16[k][i][h], 0, 0);
                }
            } else if constexpr (MASKED || RES) {
#pragma unroll
                for (int k = 0; k < NT; ++k) {
                    const int mm = RES ? 1 : ea.mask_mode(du_[k]);
                    const __amdgpu_buffer_rsrc_t rm = rsrc(RES ? ea.addsrc : (mm ? ea.mask(du_[k]) : ea.dst(du_[k])), k);
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            mk[2 * i + h][2 * k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rm, mm ? wo[k][i][h] : OOB, 0, 0));
                            mk[2 * i + h][2 * k + 1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rm, mm ? wo2(k, i, h) : OOB, 0, 0));
                        }
                }
            }
            if constexpr (BITS) {
#pragma unroll
                for (int k = 0; k < NT; ++k) mbits[k] = mbits_pre[k];
            }
            auto body = [&](auto act_tag) __attribute__((always_inline)) {
#pragma unroll
                for (int k = 0; k < NT; ++k) {
                    const __amdgpu_buffer_rsrc_t rd = DST16 ? rsrc16(ea.dst(du_[k]), k) : rsrc(ea.dst(du_[k]), k);
                    const int mm = ea.mask_mode(du_[k]);
                    const float msl = mm == 1 ? 0.2f : (mm == 0 ? 1.f : 0.f);      // act'(x <= 0); a destination without a mask (its requests came back as zeros): 1
                    unsigned sb = 0u;
                    float hp[EK == EK_HEAD ? MT * 2 : 1][4];        // (EK_HEAD) this lane's partial head sums per pixel block
                    const bool keep = EK != EK_HEAD || ea.dst0 != nullptr;      // (EK_HEAD, eval forward: the 32-channel map is not stored)
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            f32x4 o0, o1;
                            if constexpr (FWDL) {                    // (backward-data has no bias: the launcher checks)
                                o0 = take_bias(2 * i + h, 2 * k, bias4[2 * k]); o1 = take_bias(2 * i + h, 2 * k + 1, bias4[2 * k + 1]);
#pragma unroll
                                for (int c = 0; c < 4; ++c) { float e = o0[c]; act_sign(e, sb, aslope, act_tag); o0[c] = e; }
#pragma unroll
                                for (int c = 0; c < 4; ++c) { float e = o1[c]; act_sign(e, sb, aslope, act_tag); o1[c] = e; }
                            } else if constexpr (RES) {
                                // (bias from LDS at its use: the 16 registers of bias4 are what this kernel does not have beside the 64 residual words)
                                o0 = take_bias(2 * i + h, 2 * k, *reinterpret_cast<const f32x4*>(bias_lds + n0 + 32 * k + c4));
                                o1 = take_bias(2 * i + h, 2 * k + 1, *reinterpret_cast<const f32x4*>(bias_lds + n0 + 32 * k + 16 + c4));
                            } else if constexpr (BITS) {
                                const f32x4 v0 = take_raw(2 * i + h, 2 * k), v1 = take_raw(2 * i + h, 2 * k + 1);
                                // (EK_BWDU: a pixel outside the map becomes zero HERE, so that the amax slot sees exactly what is stored, as the pass's did)
                                const float fpos = UNP ? (okp[i][h] ? dsc : 0.f) : dsc, fneg = UNP ? (okp[i][h] ? dsc * msl : 0.f) : dsc * msl;
#pragma unroll
                                for (int c = 0; c < 4; ++c) o0[c] = mask_scale(v0[c], mbits[k], fpos, fneg);
#pragma unroll
                                for (int c = 0; c < 4; ++c) o1[c] = mask_scale(v1[c], mbits[k], fpos, fneg);
                            } else {
                                o0 = take(2 * i + h, 2 * k); o1 = take(2 * i + h, 2 * k + 1);
                            }
                            if constexpr (MASKED) {
                                const f32x4 m1 = mk[2 * i + h][2 * k], m2 = mk[2 * i + h][2 * k + 1], mx = ror8(sel(lo8, m2, m1));
                                const f32x4 q0 = sel(lo8, m1, mx), q1 = sel(lo8, mx, m2);      // the masks of this lane's lower / upper block
                                const f32x4 t0 = o0 * msl, t1 = o1 * msl;
#pragma unroll
                                for (int c = 0; c < 4; ++c) { o0[c] = q0[c] > 0.f ? o0[c] : t0[c]; o1[c] = q1[c] > 0.f ? o1[c] : t1[c]; }
                            }
                            if constexpr (RES16) {
                                // the residual word holds the halves as pack16 leaves them: the swap is an involution, so swapping its dwords back gives this lane's
                                // own two quads (lower / upper 16-column block); widened exactly, added to the float32 sums, then ONE rounding in pack16
                                typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
                                const u32x4 rw = mk16[2 * i + h][k];
                                const auto u0 = __builtin_amdgcn_permlane16_swap(rw.x, rw.z, false, false), u1 = __builtin_amdgcn_permlane16_swap(rw.y, rw.w, false, false);
                                const f16x2 r00 = __builtin_bit_cast(f16x2, (unsigned)u0[0]), r01 = __builtin_bit_cast(f16x2, (unsigned)u1[0]);
                                const f16x2 r10 = __builtin_bit_cast(f16x2, (unsigned)u0[1]), r11 = __builtin_bit_cast(f16x2, (unsigned)u1[1]);
                                o0 += f32x4{(float)r00.x, (float)r00.y, (float)r01.x, (float)r01.y};
                                o1 += f32x4{(float)r10.x, (float)r10.y, (float)r11.x, (float)r11.y};
                                track(o0); track(o1);
                                __builtin_amdgcn_raw_buffer_store_b128(pack16(o0, o1), rd, wo16[k][i][h], 0, CONVS_STORE_AUX);
                                __builtin_amdgcn_sched_barrier(0);
                                continue;
                            } else if constexpr (RES) {                // trade first, then add what the two store instructions' addresses hold of the residual
                                trade(o0, o1);
                                o0 += mk[2 * i + h][2 * k]; o1 += mk[2 * i + h][2 * k + 1];
                                track(o0); track(o1);
                                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o0), rd, wo[k][i][h], 0, CONVS_STORE_AUX);
                                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o1), rd, wo2(k, i, h), 0, CONVS_STORE_AUX);
                                continue;
                            }
                            if constexpr (UNP) {
                                // trade first, then add what the pooled map's gradient holds for the two store addresses: window position kp = 2 (y & 1) + (x & 1)
                                // = 2 i + (lane & 1) (tiles start at even pixels), o = (kp == argmax) ? g x (element kp > 0 ? 1 : slope) : 0, v = t + o -- also when o is zero
                                trade(o0, o1);
                                const unsigned kp = 2u * i + (unsigned)(lane_e & 1);
                                auto unpool = [&](f32x4& t, const f32x4 g4, const unsigned cw) __attribute__((always_inline)) {
                                    const unsigned sg = cw >> kp;            // bit 8 c + 2: the sign of this pixel's window element of channel c
#pragma unroll
                                    for (int c = 0; c < 4; ++c) {
                                        const float d = ((sg >> (8 * c + 2)) & 1u) ? 1.f : msl;
                                        const float m = __fmul_rn(g4[c], d);
                                        t[c] = __fadd_rn(t[c], (((cw >> (8 * c)) & 3u) == kp) ? m : 0.f);
                                    }
                                };
                                unpool(o0, pg_pre[k][h][0], pc_pre[k][h][0]); unpool(o1, pg_pre[k][h][1], pc_pre[k][h][1]);
                                track(o0); track(o1);
                                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o0), rd, wo[k][i][h], 0, CONVS_STORE_AUX);
                                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o1), rd, wo2(k, i, h), 0, CONVS_STORE_AUX);
                                continue;
                            }
                            track(o0); track(o1);
                            if constexpr (EK == EK_HEAD) {
#pragma unroll
                                for (int o = 0; o < 4; ++o) {
                                    float sacc = hw[2 * o].x * o0.x;
                                    sacc = __builtin_fmaf(hw[2 * o].y, o0.y, sacc); sacc = __builtin_fmaf(hw[2 * o].z, o0.z, sacc); sacc = __builtin_fmaf(hw[2 * o].w, o0.w, sacc);
                                    sacc = __builtin_fmaf(hw[2 * o + 1].x, o1.x, sacc); sacc = __builtin_fmaf(hw[2 * o + 1].y, o1.y, sacc);
                                    sacc = __builtin_fmaf(hw[2 * o + 1].z, o1.z, sacc); sacc = __builtin_fmaf(hw[2 * o + 1].w, o1.w, sacc);
                                    hp[i * 2 + h][o] = sacc;
                                }
                                if (!keep) continue;
                            }
                            if constexpr (DST16) {
                                __builtin_amdgcn_raw_buffer_store_b128(pack16(o0, o1), rd, wo16[k][i][h], 0, CONVS_STORE_AUX);
                                __builtin_amdgcn_sched_barrier(0);      // (one block pair at a time, as the float32 pattern's trade orders them: interleaved, the 64-column kernel spills)
                                continue;
                            }
                            trade(o0, o1);
                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o0), rd, wo[k][i][h], 0, CONVS_STORE_AUX);
                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o1), rd, wo2(k, i, h), 0, CONVS_STORE_AUX);
                        }
                    if constexpr (EK == EK_HEAD) {
                        // the 4 lanes of a pixel (q = lane >> 4) add their partial sums: exchange with lane ^ 16 (each keeps two outputs), then with
                        // lane ^ 32 (each keeps one): lane q ends with output o = 2 (q & 1) + (q >> 1) of its pixel, summed in a fixed order
                        const int q = lane_e >> 4, a16 = (lane_e ^ 16) * 4, a32 = (lane_e ^ 32) * 4;
                        const bool q0 = q & 1, q1 = q >> 1;
                        const int oo = 2 * (q & 1) + (q >> 1);
                        const float hb = head_lds[128 + oo];
                        const int64_t plane = (int64_t)ea.OH * ea.OW;
                        float* outp = ea.head_out + ((int64_t)b * 4 + oo) * plane;
                        const float* resp = ea.head_res ? ea.head_res + ((int64_t)b * 4 + oo) * plane : nullptr;
#pragma unroll
                        for (int blk = 0; blk < MT * 2; ++blk) {
                            const float s0 = q0 ? hp[blk][0] : hp[blk][2], s1 = q0 ? hp[blk][1] : hp[blk][3];
                            const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(a16, __builtin_bit_cast(int, s0)));
                            const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(a16, __builtin_bit_cast(int, s1)));
                            const float k0 = (q0 ? hp[blk][2] : hp[blk][0]) + r0, k1 = (q0 ? hp[blk][3] : hp[blk][1]) + r1;
                            const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(a32, __builtin_bit_cast(int, q1 ? k0 : k1)));
                            float v = (q1 ? k1 : k0) + r2 + hb;
                            const int i = blk >> 1, h = blk & 1;
                            if (okp[i][h]) {
                                const int64_t off = (int64_t)(py0 + i) * ea.OW + px0 + 16 * h;
                                if (resp) v += resp[off];
                                outp[off] = v;
                            }
                        }
                    }
                    if constexpr (FWDL && Scheme::BITS) {
                        const __amdgpu_buffer_rsrc_t rb = bits_rsrc(ea.bits_out, ea.nblk0);
                        if (keep) __builtin_amdgcn_raw_buffer_store_b32(sb, rb, (ea.bits_out && blk_[k] && !du_[k]) ? bits_off(k, ea.nblk0) : OOB, 0, 0);
                    }
                    track_done(du_[k]);
                }
            };
            // one wave-uniform branch per tile: with / without an activation (backward-data never has one: the launcher sends a masked layer
            // WITH an activation to the general kernel)
            if constexpr (!FWDL) body(std::false_type{});
            else if constexpr (DST16) body(std::true_type{});      // (no branch: without an activation the slope is 1 and max(o, 1 o) = o bit for bit.  With two copies
                                                                    // the compiler hoists their common 64 fma in front of the branch and the 64-column kernel spills)
            else if (ea.act != 0) body(std::true_type{});
            else body(std::false_type{});
            return;
        }
        // ---- the general case (residual, accumulation), branch-free as well: what a block does not use is requested out of range
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const int du = du_[k], mm2 = ea.mask_mode(du), acc2 = ea.accum(du);
            const bool use_add2 = ea.addsrc && du == 0;
            const __amdgpu_buffer_rsrc_t rd = rsrc(ea.dst(du), k);
            const __amdgpu_buffer_rsrc_t rm = rsrc(mm2 ? ea.mask(du) : ea.dst(du), k);
            const __amdgpu_buffer_rsrc_t rad = rsrc(use_add2 ? ea.addsrc : ea.dst(du), k);
            const float msl = mm2 == 1 ? 0.2f : (mm2 == 0 ? 1.f : 0.f);
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                f32x4 m2[MT][2], ad2[MT][2], pr2[MT][2];
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        m2[i][h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rm, mm2 ? vo[k][i][h] : OOB, jj * 64, 0));
                        ad2[i][h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rad, use_add2 ? vo[k][i][h] : OOB, jj * 64, 0));
                        pr2[i][h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rd, acc2 ? vo[k][i][h] : OOB, jj * 64, 0));
                    }
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        f32x4 o = act4(take(2 * i + h, 2 * k + jj) + bias4[2 * k + jj] + ad2[i][h]);
                        const f32x4 t = o * msl;
#pragma unroll
                        for (int c = 0; c < 4; ++c) o[c] = m2[i][h][c] > 0.f ? o[c] : t[c];
                        o += pr2[i][h];
                        track(o);
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rd, vo[k][i][h], jj * 64, 0);
                    }
            }
            track_done(du);
        }
    };

    // ---- the consumers' loop: barrier, item, barrier, item, ...  (no vector-memory wait anywhere: the only operations a consumer has in
    // flight are its own epilogue's and the prefetches for it, and nothing in the K loop depends on them)
    int img = 0, st = 0;
#ifdef CONVS_STAMPS
    long long t_mfma = 0, t_epi = 0, t_bar = 0, tlast_ = clock64(), tall = tlast_; int nch = 0;
#endif
    CS_BARRIER();                                                 // barrier 0
    CS_T(t_bar)
    if constexpr (EK == EK_HEAD) {
#pragma unroll
        for (int q = 0; q < 8; ++q) hw[q] = *reinterpret_cast<const f32x4*>(head_lds + (q >> 1) * 32 + (q & 1) * 16 + (lane >> 4) * 4);
    }
    for (;;) {
        const Ck n1 = chunk_at(K1{});
#ifdef CONVS_STAMPS
        ++nch;
#endif
        if constexpr (EK == EK_BWDB || EK == EK_BWDU) { if (g == nchunks - 1) prefetch_bits(cur); }
        if constexpr (EK == EK_BWDU) { if (g == nchunks - 1) prefetch_pool(cur); }
        static_for<0, ITEMS>([&](auto rt) {
            constexpr int r = decltype(rt)::value;
            const int im = img, ws = stage_after(st, r);          // (named in this order: the register allocation of the parent kernel text)
            Scheme::template mfma_item<BN>(acc, xs, wsb, wave, lane, r, ws, im);
            CS_T(t_mfma)
            if constexpr (r + 1 < ITEMS) {
                CS_BARRIER();
                CS_T(t_bar)
            }
        });
        const bool last_chunk = g == nchunks - 1;
        if (last_chunk) epilogue(cur);
        CS_T(t_epi)
        if (!n1.ok) break;
        CS_BARRIER();
        CS_T(t_bar)
        if (last_chunk) next_tile(); else ++g;
        img ^= 1; st = stage_after(st, ITEMS);
    }
    // ---- max |stored value| of the wave per destination -> the amax slots (non-negative floats order like their bit patterns)
    if constexpr (Scheme::SCALED) {
#pragma unroll
        for (int du = 0; du < 2; ++du) {
            if (!ha.amax_out[du]) continue;
            pnnp_amax_commit(du ? amx1 : amx0, ha.amax_out[du]);
        }
    }
#ifdef CONVS_STAMPS
    __builtin_amdgcn_s_waitcnt(0x0f70);
    if (lane == 0) {
        float* d = a.dst[0] + ((int64_t)blockIdx.x * (NCW + NPW) + wave) * 8;
        d[0] = (float)t_mfma; d[1] = (float)t_epi; d[2] = (float)t_bar; d[3] = 0.f; d[4] = (float)(clock64() - tall); d[5] = (float)nch;
    }
#endif
