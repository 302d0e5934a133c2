// dq_h_body.inc -- the body of dq_h_kernel (dqgemm_v2.h), textually shared by the one-problem kernel `dq_h_kernel(K2Args A)` and the
// grouped one `dq_hg_kernel(K2GArgs G)` (blockIdx.y picks the problem): the SAME text compiled twice, so that the headline kernel's
// generated code does not move when the grouped form is built (tests/test_k2_isa.py audits both).  Expects `A` (K2Args) in scope and the
// template parameters BITS, ACT, RT, NW, NCH, HALF, EXACT.
    // The dequantiser.  Multi-exponent (dq_common.h, DeqME2: 10 VALU per packed dword instead of 16) for the 2-bit forms of 4 waves x 4 chunks --
    // d = 4096: the headline, its half-slab twin, RT 2 / 4, ragged K, the grouped kernel.  There a wave runs one chain of 32 MFMA steps, one wave
    // per SIMD, and the chunk interval is its own instruction stream (profiles/k2h_pipeline.md section 4, profiles/k2h_me.md).  The offset of a
    // dequantised value then depends on k, so the meet needs S_off = sum_k OFF_k x beside S_1 = sum_k x: both come from the ONE row-sum MFMA of
    // a step (`sfr` below).  Every other form keeps the uniform offset: with 8 or 16 steps per wave the constants and the two fragments cost
    // more instructions than the shifts they save (8 x 1: 311 against 268 in all), and the fp32 sums carry offsets of 128 / 64 instead of 4
    // (1e-5 instead of 1e-6 relative on y), which the last-bit comparisons of the d = 2048 forms with the fused operator kernel
    // (tests/test_gpu_method.py) do not allow.  -DK2_H_UNIFORM=1 (lab builds, scripts/k2lab.hip; default in dqgemm_v2.h): uniform everywhere.
#if K2_H_UNIFORM
    typedef DeqUni<BITS, ACT> Q;
#else
    typedef typename std::conditional<NW == 4 && NCH == 4, DeqSel<BITS, ACT>, DeqUni<BITS, ACT>>::type Q;
#endif
    constexpr int KC = Q::KC, NT = Q::NT;
    // HALF (bs <= 8): a slab holds rows 0..7 only -- 1 KiB per 128-byte column block instead of 2 -- and lanes j >= 8 read the rows of j - 8
    // (their batch columns are never stored).  Half the LDS: d = 8192 (32 chunks) fits a workgroup at bs <= 8 (round 6: OPT's fc2 in a blocked
    // decode step ran on the round-1 tile kernel, 6.6 us).
    constexpr int ROWB = KC * 2, NCB = ROWB / 128, NI = 2 * NCB, CBS = HALF ? 1024 : 2048, XB = NCB * CBS;
    // (negative result, profiles/r02d_k2lab.log: loading half of the B fragments straight into registers, to use a second
    //  return path beside the ~28 B/clk/CU LDS-DMA path, made the launch 0.9 us SLOWER)
    constexpr int NDMA = HALF ? NI / 2 : NI, OPC = RT + NDMA;         // vector-memory operations per chunk
    static_assert((NCH - 1) * OPC < 64, "vmcnt range");
    static_assert(RT * 1024 + 128 <= NCH * XB, "a wave parks its partials and its two row sums in its own slab region");
    extern __shared__ __attribute__((aligned(16))) char smem[];     // [NW][NCH] slabs; a wave parks its partials in its own
    const EpiArgs &e = A.e;
    // (round 3, negative result, scripts/k2_ab.sh on one box, alternating runs: WAITING for all fifteen kernarg fields in one scalar round
    //  trip up front -- the fix that took 2000 cycles off the prologue of csrc/decode_fused.hip -- made this kernel 0.13 us slower than the
    //  lazily fetched head it had then.  The head is now K2_HEAD below: the weight requests need qw and d only, which arrive preloaded in the
    //  one-problem kernel and in one round trip in the grouped one; nothing waits for the other fields in front of the tiles.)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    K2_STAMP(0);
    QA_LOG(0)
    const int j = lane & 15, g = lane >> 4;
    const uint32_t nkc = (uint32_t)(A.d / KC);
    const uint32_t rt0 = blockIdx.x * RT;

    // Which k-chunks a wave owns (round 5).  Rounds 2-4: wave w owns chunks w, w + NW, ... in every workgroup.  scripts/xingest_lab.hip
    // (profiles/r05d / r05e_xingest_lab.txt) timed the ingest of x alone -- 128 KiB into every CU of a 256-workgroup launch: 4091-4790
    // clocks in that order, 2775-3600 with the order rotated by the workgroup's index inside its XCD (blockIdx.x >> 3; the 32 CUs of an XCD
    // otherwise walk x in lockstep and queue on the same L2 channels), 3266 with a wave's chunks ADJACENT (NCH w + i: one contiguous run of x
    // per row and of weight tiles per wave) -- against 2048 at the L1 return rate.  In the kernel itself (scripts/k2lab.hip builds with
    // -DK2_CHUNKS, alternating on one box, profiles/r05f_k2lab_chunks_fine_ab.txt): adjacent 3.66 us warm against 4.18 (cold 4.72 against
    // 4.77: there the weights' HBM round trip is what lands last, see K2_WFIRST below); rotation alone 3.96; both 3.71.  Default: adjacent.
    // The set of chunks a workgroup sums is unchanged; only which wave holds which partial (the order of the fp32 meet) moves.
    // K2_CHUNKS (lab builds, scripts/k2lab.hip): 0 = wave w owns chunks w, w + NW, ... in every workgroup (rounds 2-4); 1 = that, rotated;
    // 2 = a wave's chunks ADJACENT (NCH w + i: its x slabs and its weight tiles are contiguous runs), 3 = adjacent and rotated
#ifndef K2_CHUNKS
#define K2_CHUNKS 2
#endif
    const uint32_t rot = (EXACT && (K2_CHUNKS & 1)) ? (uint32_t)(blockIdx.x >> 3) : 0u;
    auto chunk_of = [&](int i) -> uint32_t {
        if (!EXACT) return (uint32_t)(i * NW + wave);
        return ((K2_CHUNKS & 2) ? (uint32_t)(NCH * wave + i) + NCH * rot : (uint32_t)(i * NW + wave) + rot) & (uint32_t)(NW * NCH - 1);
    };
    static_assert((NW * NCH & (NW * NCH - 1)) == 0, "chunk slots: a power of two");
    // ---- request everything --------------------------------------------------------------------------------------------
    // K2_WFIRST (round 5): the weight tiles of ALL chunks go out before the first x slab.  They come from HBM (the cold regime: ~2000 clocks),
    // x from the L2s; behind a chunk's eight DMA instructions -- which queue on the CU's one vector-memory path -- the next chunk's weight
    // request left ~1500 clocks late and was the last thing to land.  Memory returns in order, so the counted waits become
    // "all weights + the slabs up to mine": (NCH - 1 - i) slabs may be outstanding.
#ifndef K2_WFIRST
#define K2_WFIRST 1
#endif
    constexpr bool WFIRST = EXACT && (K2_WFIRST != 0);
    // K2_AHEAD (issue-ahead schedule): "request everything, then consume" keeps a wave in the ISSUE of its NCH * NDMA LDS-DMA instructions
    // until the CU's vector-memory queue has drained that far (clock ~3900 of the headline launch, profiles/r06g_k2h_stamps_insitu.txt), and
    // only then does it start its ~690 clocks per chunk of ds_read + dequant + MFMA: the four SIMDs idle through the ingest and do all their
    // arithmetic behind it.  With AHEAD < NCH the prologue requests the weight tiles and the slabs of the first AHEAD chunks only; DMA
    // instruction t of chunk i + AHEAD goes out in front of MFMA step t of chunk i (NI == NT: one instruction per step, 1 KiB of x against
    // ~85 clocks of instructions; HALF: the even steps only).  Memory returns in order, so the counted wait in front of chunk i is "the
    // slabs requested behind mine": chunks i + 1 .. min(i + AHEAD - 1, NCH - 1).  A slab is written once and never reused, so nothing guards
    // a write after a read.  AHEAD = NCH is the old instruction stream exactly.  The arithmetic (MFMA order, the two chains, the meet) does
    // not move: y is bit-identical for every AHEAD.  Measured: profiles/k2h_pipeline.md.
    // Which instantiations: the headline <2, RT 1, 4 x 4> (HALF or not) of the one-problem kernel; every other one keeps AHEAD = NCH until an
    // A/B on its own shape shows a gain.  -DK2_AHEAD=n (lab builds, scripts/k2lab.hip) forces n on EVERY exact instantiation.
#ifdef K2_AHEAD
    constexpr int AHEAD = WFIRST ? ((K2_AHEAD) < 1 ? 1 : (K2_AHEAD) > NCH ? NCH : (K2_AHEAD)) : NCH;
#else
    constexpr int AHEAD = (WFIRST && !K2_GROUPED && BITS == 2 && RT == 1 && NW == 4 && NCH == 4) ? 2 : NCH;
#endif
    static_assert(NI == NT, "one LDS-DMA instruction per MFMA step");
    // K2_PIN: an empty asm that names accumulators ("a": they live in AGPRs; "v" cost 512 v_accvgpr copies) -- see `pin` in the MFMA loop.
    // Device pass only: the host pass parses this body too, and "a" means something else there.
#ifndef K2_PIN
#if defined(__HIP_DEVICE_COMPILE__)
#define K2_PIN(x) asm volatile("" : "+a"(x))
#define K2_PIN2(x, y) asm volatile("" : "+a"(x), "+a"(y))
#else
#define K2_PIN(x) (void)(x)
#define K2_PIN2(x, y) (void)(x), (void)(y)
#endif
#endif
    // ---- the head of the wave (K2_HEAD, profiles/k2h_head.md) ---------------------------------------------------------------------------
    // The cold critical path is wave start -> kernel arguments -> weight request -> HBM round trip -> chunk 0 -> ... -> store: whatever sits in
    // front of the weight request delays the whole launch by as much.  So the weight tiles are the wave's FIRST vector-memory instructions and
    // only what their addresses need (qw, d) is read in front of them.  The epilogue parameters (first used behind the meet) are requested
    // between the weight tiles and the first x slab: still in front of every slab, so no counted wait changes -- the waits count the
    // operations behind a chunk's slab.  K2_HEAD_PIN: hipcc's scheduler moves scalar arithmetic (and the s_waitcnt lgkmcnt its operands need)
    // freely across the asm loads; the two fields the code right behind the weight tiles reads (qfn: which epilogue loads; bs: the extent of
    // x's descriptor) pass through an empty asm, and volatile asms keep their order.  The "memory" clobbers keep the epilogue loads between
    // the weight tiles and the LDS-DMA builtins.  -DK2_HEAD=0 (lab builds): the old order -- epilogue parameters, then the weight tiles.
#ifndef K2_HEAD
#define K2_HEAD 1
#endif
#ifndef K2_HEAD_PIN
#if defined(__HIP_DEVICE_COMPILE__)
#define K2_HEAD_PIN(q, b) asm volatile("" : "+s"(q), "+s"(b) : : "memory")
#define K2_HEAD_FENCE() asm volatile("" : : : "memory")
#define K2_HEAD_ARG(p) asm volatile("" : "+s"(p))
#else
#define K2_HEAD_ARG(p) (void)(p)
#define K2_HEAD_PIN(q, b) (void)(q), (void)(b)
#define K2_HEAD_FENCE() (void)0
#endif
#endif
    int h_qfn = e.qfn;
    int64_t h_bs = e.bs;
    // reducer role u = 4*r2 + q (below): the epilogue parameters of this wave's first role
    float e_sc = 0.f, e_zr = 0.f, e_bi = 0.f;
    auto request_epi = [&]() {
        if (wave < 4 * RT) {
            const int64_t row = (int64_t)(rt0 + (wave >> 2)) * 16 + (lane & 15);
            e_sc = h_qfn == QUIPAMD_QFN_B ? e.scale[0] : e.scale[row];
            if (h_qfn != QUIPAMD_QFN_B) e_zr = e.zero[row];
            if (e.bias) e_bi = e.bias[row];
        }
        K2_HEAD_FENCE();
    };
    if constexpr (K2_HEAD == 0) request_epi();
    u32x4 w[NCH][RT];
    K2_STAMP2(12);                                                    // in front of the first weight request
    if constexpr (WFIRST) {
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int r = 0; r < RT; ++r) load_w_nt(w[i][r], A.qw + ((uint64_t)(rt0 + r) * nkc + chunk_of(i)) * 64 + lane);
    } else if constexpr (K2_HEAD != 0) {                              // chunk by chunk: the first chunk's tiles (the loop below skips them)
        const u32x4 *qw0 = A.qw;
        K2_HEAD_ARG(qw0);                                             // read with d, in ONE round trip: not inside the branch, behind d
        if (EXACT || chunk_of(0) < nkc) {
#pragma unroll
            for (int r = 0; r < RT; ++r) load_w_nt(w[0][r], qw0 + ((uint64_t)(rt0 + r) * nkc + chunk_of(0)) * 64 + lane);
        }
    }
    if constexpr (K2_HEAD != 0) {
        K2_HEAD_PIN(h_qfn, h_bs);
        request_epi();
    }

    const uint32_t rowbytes = (uint32_t)A.d * 2u;
    char *myreg = smem + wave * (NCH * XB);
    __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void *)A.x, 0, (int)(h_bs * (int64_t)rowbytes), 0x00020000);
    const uint32_t voff_lo = (lane >> 3) * rowbytes + ((uint32_t)((lane & 7) ^ (lane >> 3)) << 4);
    const uint32_t voff_hi = voff_lo + 8u * rowbytes;
    const uint32_t rd_base = lds_addr(myreg) + (HALF ? 0 : (j >> 3) * 1024) + (j & 7) * 128;
    const uint32_t rd0 = rd_base + (((0 + g) ^ (j & 7)) << 4);        // even MFMA steps
    const uint32_t rd1 = rd_base + (((4 + g) ^ (j & 7)) << 4);        // odd MFMA steps
    // DMA instruction q of chunk i, for the requests between the MFMA steps.  (Its call in the chunk loop is compiled in the device pass only:
    // the host pass, which parses this body too, takes the call inside the generic lambda as an error it never prints and then cannot form
    // the kernel's address for qa_lds<> -- "cannot compile this l-value expression yet".)
    auto dma = [&](int i, int q) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (lds_void2_t *)(myreg + i * XB + (q >> 1) * CBS + (q & 1) * 1024), 16, (q & 1) ? voff_hi : voff_lo,
                                                 chunk_of(i) * ROWB + (q >> 1) * 128, 0, 0);
    };
#pragma unroll
    for (int i = 0; i < AHEAD; ++i) {
        const uint32_t kc = chunk_of(i);
        if (EXACT || kc < nkc) {                                      // wave-uniform
            if constexpr (!WFIRST) {
            if (K2_HEAD == 0 || i > 0) {
#pragma unroll
            for (int r = 0; r < RT; ++r) load_w_nt(w[i][r], A.qw + ((uint64_t)(rt0 + r) * nkc + kc) * 64 + lane);
            }
            }
#pragma unroll
            for (int q = 0; q < NI; ++q) {
                if ((q & 1) && HALF) continue;                        // rows 8..15 of a slab feed batch columns never stored
                __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (lds_void2_t *)(myreg + i * XB + (q >> 1) * CBS + (q & 1) * 1024), 16, (q & 1) ? voff_hi : voff_lo,
                                                         kc * ROWB + (q >> 1) * 128, 0, 0);
            }
        }
        // (a chunk past the end of a ragged K: its w[i] is never read, the chunk loop skips it.  It used to be zeroed here; that join of an asm
        //  load with a constant is a copy hipcc may place BEFORE the load's data has landed -- tests/test_k2_isa.py caught it once the head moved)
    }

    K2_STAMP(1);
    // two accumulator chains each (even / odd MFMA steps): a dependent MFMA behind other instructions costs ~60 cycles
    // (MI355X_MICROARCH.md "one EXTRA issue slot between two MFMAs on the SAME accumulator"), an independent one 16
    f32x4_t acc[RT][2], accx[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r][0] = acc[r][1] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // The row-sum A fragments, made ONCE per wave and behind every request of the prologue (the head of the wave does not grow).  Multi-exponent:
    // A row 0 = ones, row 1 = the OFF_k pattern of the step's parity, the other rows zero, so D[0][b] = S_1 and D[1][b] = S_off from one product
    // (the construction of dq_mb_kernel, dqgemm_v2.h); uniform: ones in every row, as before.
    const typename Q::Consts qc = Q::make_consts();
    const u32x4 ones = {opaque(ACT::ONES), opaque(ACT::ONES), opaque(ACT::ONES), opaque(ACT::ONES)};
    u32x4 sfr[2] = {ones, ones};
    if constexpr (!Q::UNIFORM) {
        const u32x4 zero4 = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 2; ++k) sfr[k] = j == 0 ? ones : (j == 1 ? Q::off_frag(k, qc) : zero4);
    }
    // K2_PREFETCH (lab option): the eight ds_read_b128 of chunk i + 1 go out in front of the MFMA steps of chunk i, into the other of two fragment
    // buffers (one wave per SIMD: registers to spare), so their LDS latency hides under arithmetic.  The counted wait for chunk i + 1's slab moves
    // in front of chunk i's arithmetic with them.  Measured on top of K2_AHEAD: profiles/k2h_pipeline.md.
#ifndef K2_PREFETCH
#define K2_PREFETCH 0
#endif
    constexpr bool PREF = WFIRST && (K2_PREFETCH != 0) && AHEAD >= 2;     // chunk i + 1 must be in the queue while chunk i is consumed
    u32x4 xfa[NT], xfb[NT];
    static_for<NCH>([&](auto I) {
        constexpr int i = decltype(I)::value;
        const uint32_t kc = chunk_of(i);
        if (EXACT || kc < nkc) {
            // K2_FINE (round 5, lab option, OFF: a negative result): the LAST chunk of a wave consumed column block by column block -- MFMA steps
            // 2 cb, 2 cb + 1 read the 128-byte column block cb of the slab = DMA instructions 2 cb (rows 0..7) and 2 cb + 1 (rows 8..15), so each
            // pair of steps waits only for the instructions in front of it, and behind the last byte of x the wave has two steps of dequant +
            // MFMA left, not eight.  Measured (profiles/r05f_k2lab_chunks_fine_ab.txt): cold -0.03 us, warm +0.05: the tail of the chain is the
            // meet (park, barrier, reduce, store), not the last chunk's arithmetic.
#ifndef K2_FINE
#define K2_FINE 0
#endif
            constexpr bool FINE = EXACT && (K2_FINE != 0) && i == NCH - 1 && NT == 2 * NCB;
            constexpr int OPL = WFIRST ? NDMA : OPC;                  // operations a LATER chunk has in the queue behind mine
            constexpr int LAST = i + AHEAD - 1 < NCH - 1 ? i + AHEAD - 1 : NCH - 1;    // the last chunk whose slab is in the queue behind mine
            constexpr int NWAIT = EXACT ? (LAST - i) * OPL + (FINE ? NDMA - (HALF ? 1 : 2) : 0) : 0;    // ragged K: everything, then compute
            constexpr int NXT = i + AHEAD;                            // the chunk whose slab is requested under this chunk's MFMA steps
            constexpr int PWAIT = (LAST - i - 1) * OPL;              // PREF: chunk i + 1 has landed; chunk NXT is requested behind this wait
            if constexpr (AHEAD < NCH && i > 0) {                     // the arithmetic of chunk i - 1 stays in front of this wait (see `pin` below)
#pragma unroll
                for (int r = 0; r < RT; ++r) K2_PIN2(acc[r][0], acc[r][1]);
                K2_PIN2(accx[0], accx[1]);
            }
            if constexpr (i == 0 || !PREF) {
            if constexpr (i < 4) K2_STAMP2(8 + i);
            if constexpr (RT == 1) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(w[i][0]) : "n"(NWAIT) : "memory");
            else if constexpr (RT == 2) asm volatile("s_waitcnt vmcnt(%2)" : "+v"(w[i][0]), "+v"(w[i][1]) : "n"(NWAIT) : "memory");
            else {
                static_assert(RT == 1 || RT == 2 || RT == 4, "row tiles per wave");
                asm volatile("s_waitcnt vmcnt(%4)" : "+v"(w[i][0]), "+v"(w[i][1]), "+v"(w[i][2]), "+v"(w[i][RT - 1]) : "n"(NWAIT) : "memory");
            }
            if constexpr (i > 0 && i < 4) K2_STAMP2(12 + i);  // (chunk 0: slot 2, right below; slot 12 is the head's)
            }
            if constexpr (i == 0) K2_STAMP(2);
            if constexpr (i == NCH - 1) K2_STAMP(3);
            if constexpr (FINE) {
                static_assert(!PREF, "K2_FINE and K2_PREFETCH: one or the other");
                static_for<NCB>([&](auto CB) {
                    constexpr int cb = decltype(CB)::value;
                    if constexpr (cb > 0) wait_vm<(NCH - 1 - i) * OPL + NDMA - (HALF ? 1 : 2) * (cb + 1)>();
                    u32x4 xp[2];
                    lds_read16<i * XB + cb * CBS>(xp[0], rd0);
                    lds_read16<i * XB + cb * CBS>(xp[1], rd1);
                    wait_lgkm(xp);
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
#pragma unroll
                        for (int r = 0; r < RT; ++r) acc[r][h] = ACT::mfma(Q::frag(w[i][r], 2 * cb + h, qc), xp[h], acc[r][h]);
                        accx[h] = ACT::mfma(sfr[h], xp[h], accx[h]);
                    }
                });
            } else {
            u32x4 xfl[NT];
            u32x4 (&xf)[NT] = !PREF ? xfl : (i & 1) ? xfb : xfa;
            if constexpr (i == 0 || !PREF) {
            static_for<NT>([&](auto T) {
                constexpr int t = decltype(T)::value;
                lds_read16<i * XB + (t >> 1) * CBS>(xf[t], (t & 1) ? rd1 : rd0);
            });
            }
            wait_lgkm(xf);
            if constexpr (PREF && i + 1 < NCH) {                      // the fragments of chunk i + 1, under this chunk's arithmetic
                u32x4 (&xn)[NT] = (i & 1) ? xfa : xfb;
                if constexpr (i + 1 < 4) K2_STAMP2(8 + i + 1);
                if constexpr (RT == 1) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(w[i + 1][0]) : "n"(PWAIT) : "memory");
                else if constexpr (RT == 2) asm volatile("s_waitcnt vmcnt(%2)" : "+v"(w[i + 1][0]), "+v"(w[i + 1][1]) : "n"(PWAIT) : "memory");
                else asm volatile("s_waitcnt vmcnt(%4)" : "+v"(w[i + 1][0]), "+v"(w[i + 1][1]), "+v"(w[i + 1][2]), "+v"(w[i + 1][RT - 1]) : "n"(PWAIT) : "memory");
                if constexpr (i + 1 < 4) K2_STAMP2(12 + i + 1);
                static_for<NT>([&](auto T) {
                    constexpr int t = decltype(T)::value;
                    lds_read16<(i + 1) * XB + (t >> 1) * CBS>(xn[t], (t & 1) ? rd1 : rd0);
                });
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                // pin (AHEAD < NCH only; no instruction): hipcc's scheduler moves MFMAs freely across the asm waits and the DMA requests -- it sank a
                // whole chunk's arithmetic below the NEXT chunk's vmcnt wait and issued the eight requests in one clump.  An empty asm that names
                // this step's accumulators sits behind MFMA step t - 2 and in front of step t, and keeps its place among the requests and waits.
                if constexpr (AHEAD < NCH) {
#pragma unroll
                    for (int r = 0; r < RT; ++r) K2_PIN(acc[r][t & 1]);
                    K2_PIN(accx[t & 1]);
                }
#if defined(__HIP_DEVICE_COMPILE__)
                if (NXT < NCH && !((t & 1) && HALF)) dma(NXT, t);    // K2_AHEAD: one request per MFMA step
#endif
#pragma unroll
                for (int r = 0; r < RT; ++r) acc[r][t & 1] = ACT::mfma(Q::frag(w[i][r], t, qc), xf[t], acc[r][t & 1]);
                accx[t & 1] = ACT::mfma(sfr[t & 1], xf[t], accx[t & 1]);   // row sums of x on the matrix pipe: D[0][b] = S_1, D[1][b] = S_off
            }
            }
        }
    });
    K2_STAMP(4);

    // ---- meet: the NW k-partials of every tile ---------------------------------------------------------------------------
    {
        float *p = reinterpret_cast<float *>(myreg);                  // [RT][4][64] accumulator components, then [16] S_1 and [16] S_off
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const f32x4_t a = acc[r][0] + acc[r][1];
            p[r * 256 + lane] = a[0]; p[r * 256 + 64 + lane] = a[1];
            p[r * 256 + 128 + lane] = a[2]; p[r * 256 + 192 + lane] = a[3];
        }
        if (lane < 16) {                                              // lanes 0..15 hold D rows 0..3 of batch column `lane`
            p[RT * 256 + lane] = accx[0][0] + accx[1][0];
            if constexpr (!Q::UNIFORM) p[RT * 256 + 16 + lane] = accx[0][1] + accx[1][1];
        }
    }
    K2_STAMP(5);
    __syncthreads();
    K2_STAMP(6);
    // 4*RT reducer roles; role u = 4*r2 + q finishes batch rows 4q .. 4q+3 x the 16 weight rows of tile r2: lane l -> batch
    // row b = 4q + (l>>4), weight row l&15 (16 consecutive outputs of y per 16 lanes) = accumulator component (l&3) of MFMA
    // lane b + 16*((l&15)>>2)
    asm volatile("" : "+v"(e_sc), "+v"(e_zr), "+v"(e_bi));            // keep the epilogue arithmetic (and its vmcnt wait) down here
#pragma unroll 1
    for (int u = wave; u < 4 * RT; u += NW) {
        const int r2 = u >> 2, q = u & 3;
        const int b = 4 * q + (lane >> 4), wr = lane & 15;
        const int src = r2 * 256 + (wr & 3) * 64 + b + 16 * (wr >> 2);
        float a = 0.f, xsum = 0.f, xoff = 0.f;
        // K2_TAIL: hipcc read the row sums, waited lgkmcnt(0), and only then issued the reads of the partials -- two LDS latencies in series on
        // the tail of every launch.  All 2 NW (multi-exponent: 3 NW) reads go out, the scheduler may move nothing across the barrier, and the sums (in the same order:
        // the arithmetic does not move) wait behind it.  -DK2_TAIL=0 (lab builds): no barrier -- hipcc's own order, as measured before.
#ifndef K2_TAIL
#define K2_TAIL 1
#endif
        float pa[NW], px[NW], po[NW];
#pragma unroll
        for (int v = 0; v < NW; ++v) {
            const float *p = reinterpret_cast<const float *>(smem + v * (NCH * XB));
            pa[v] = p[src];
            px[v] = p[RT * 256 + b];
            if constexpr (!Q::UNIFORM) po[v] = p[RT * 256 + 16 + b];
        }
#if K2_TAIL && defined(__HIP_DEVICE_COMPILE__)
        __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
        for (int v = 0; v < NW; ++v) {
            a += pa[v];
            xsum += px[v];
            if constexpr (!Q::UNIFORM) xoff += po[v];
        }
        const int64_t row = (int64_t)(rt0 + r2) * 16 + wr;
        if (b < e.bs) {
            if (u != wave) {                                          // fewer waves than reducer roles
                e_sc = e.qfn == QUIPAMD_QFN_B ? e.scale[0] : e.scale[row];
                e_zr = e.qfn == QUIPAMD_QFN_B ? 0.f : e.zero[row];
                e_bi = e.bias ? e.bias[row] : 0.f;
            }
            const float alpha = e.qfn == QUIPAMD_QFN_B ? e_sc * e.two_over_maxq : e_sc;
            float val;
            if constexpr (Q::UNIFORM) {
                const float c0 = e.qfn == QUIPAMD_QFN_B ? Q::OFF + 0.5f * (float)e.maxq : Q::OFF + e_zr;
                val = alpha * (a - c0 * xsum) + e_bi;
            } else {                                                  // sum_k q x = a - S_off; z = maxq / 2 (qfn b) or zero[row] (qfn a)
                const float z = e.qfn == QUIPAMD_QFN_B ? 0.5f * (float)e.maxq : e_zr;
                val = alpha * ((a - xoff) - z * xsum) + e_bi;
            }
            const int64_t o = (int64_t)b * e.m + row;
            if (e.y_f32) ((float *)e.y)[o] = e.accumulate ? ((float *)e.y)[o] + val : val;
            else ((uint16_t *)e.y)[o] = e.y_f16 ? f32_to_f16_bits(val) : f32_to_bf16_bits(val);
        }
    }
    K2_STAMP(7);
    QA_LOG(1)
    K2_STAMP_FLUSH();
