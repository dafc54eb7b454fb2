// Body of gemm_fast_kernel (qs_gemm_fast.hip), included once per overload inside the kernel's braces: `g` is the kernel's
// argument, QS_FAST_PAIRS says whether it is a FastPairsArgs (triangular batch: the remap in `decode`, nothing else) or, 2, a
// FastPairsMirrorArgs (the same, and the epilogue of pair (i, j > i) also stores the tile transposed at pair (j, i)) or, 3, a
// FastUpperArgs (the column triangle of Product::upper: the n-tile's decode, the B stage's lane offset and the epilogue's
// column offsets; exact fp64 DMA forms only) or, 4, a FastPairsLowerArgs (the triangular batch whose A entries are square and
// stored on their 16 x 16 blocks (G, J >= G) only: a block (G, J < G) of pair (i, j) is fetched as block (J, G) of pair (j, i) and
// read from LDS the other way round; exact fp64 DMA forms only).  Text
// inclusion, not a shared device function: the plain batch's kernels then compile exactly as they did before the
// triangular batch existed (through a forced-inline function eight of them spilled other scalar registers).
// No include guard on purpose.

    static_assert(!CX || VEC, "a complex element is one 16-byte item");
    constexpr int NP = CX ? 2 : 1;
    constexpr int ES = CX ? 2 : 1;
    constexpr int KT = CX ? 8 : 16;
    constexpr int KS = KT / 4;
    constexpr int NT = 256;
    constexpr int BM = 32 * TM, BN = 32 * TN;
    // B rows: complex fragments are ds_read_b64 (row stride = 16 mod 32 doubles is conflict-free);
    // fp64 fragments are ds_read_b128 column PAIRS (row stride = 0 mod 32 is conflict-free)
    // A rows: fp64 pads the row to KT + 2 (stride 18: conflict-free fragment reads, tolerable writes).  complex128 (round 4): no
    // padding, the k index of a row XOR-ed with 2 ((row >> 2) & 3) instead -- a half wave of the stage WRITE (four rows x eight
    // k) then covers 32 different bank pairs, and so does a half wave of the fragment READ (sixteen rows x two k): with the
    // padded rows of rounds 1-3 (stride 10) writes of the A stage collided.  Measured (profiles/r04_pmc_c128.txt, same-box A/B
    // r04_c128_swizzle_ab.txt): SQ_LDS_BANK_CONFLICT 40 -> 31 % and 25 -> 18 % of the LDS-active cycles of the two tile forms,
    // l = 256 66.9 -> 67.5, l = 128 64.2 -> 64.6 TFLOP/s.  What is left scales with the number of A-stage writes (8 conflict
    // cycles per write instruction in both forms): the lanes a 64-bit LDS write serves together are not the half waves assumed
    // here -- open.
#ifdef QS_FAST_CX_PAD      // (A/B builds: the padded complex rows of rounds 1-3)
    constexpr bool kSwizzleA = false;
#else
    constexpr bool kSwizzleA = CX;
#endif
    // LDS-DMA staging (exact fp64 form): the destination of one wave-instruction is lane-linear (M0 + 16 x lane), so the
    // A rows cannot be padded.  They are 16 doubles = 128 bytes, and the 16-byte slot s of row r holds k-pair
    // s ^ ((r >> 1) & 7): the permutation is applied on the per-lane SOURCE address of the load and again on the fragment
    // read.  A half wave of the fragment read (sixteen rows x one k-pair) then covers all 64 banks: the eight even rows
    // fill bytes 0-127 of a bank row, the eight odd rows bytes 128-255.
    constexpr bool kDma = QS_FAST_DMA && !CX && VEC && !EDGE;
    constexpr int SA = (kSwizzleA || kDma) ? KT : KT + 2, SB = CX ? BN + 16 : BN;      // (B rows 8 mod 16 instead of 16 mod 32: measured, level)
    constexpr int EPI = (!CX && VEC) ? 2 : 1;           // tensor elements per global item
    constexpr int DPI = CX ? 1 : EPI;                   // doubles per item inside one LDS plane
    constexpr int IPR_A = KT / EPI;                     // items per A row of a stage
    constexpr int RA = NT / IPR_A;                      // A rows covered by one item step
    constexpr int NA = BM / RA;                         // items per thread, A stage
    constexpr int IPR_B = BN / EPI;                     // items per B row
    static_assert(NT % IPR_B == 0 && BM % RA == 0, "item steps cover whole rows");
    constexpr int RPS = NT / IPR_B;                     // B rows covered by one item step
    static_assert(KT % RPS == 0, "B item steps tile the stage");
    constexpr int NB = KT / RPS;
    constexpr int A_STAGE = NP * BM * SA, B_STAGE = NP * KT * SB;
    constexpr size_t ESZ = 8 * ES;
    constexpr unsigned IB = (unsigned)(EPI * ESZ);      // bytes per item
    static_assert(KS % 2 == 0, "fragment double buffering needs an even k-step count");
    static_assert(CX || TN % 2 == 0, "fp64 n-tiles come in column pairs");
    using Item = FastItem<CX || VEC>;
    using item_t = typename Item::type;

    extern __shared__ __attribute__((aligned(16))) double smem[];
    // (in doubles: where the B stages begin, and how far apart the waves' first DMA items of an item step lie -- 64 items of
    // A, one row of B; fetch_dma forms the same addresses in bytes from these)
    constexpr int B_BASE = 2 * A_STAGE, DST_A_WAVE = 64 * DPI, DST_B_WAVE = SB;
    double* As = smem;
    double* Bs = smem + B_BASE;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int nk = g.nk;
    const unsigned P = gridDim.x;                       // persistent grid (multiple of 8 unless P == total)
    // edge form: valid k-steps of a tile's last stage (KT when K is a whole number of stages)
    const int k_tail = EDGE ? g.k - (nk - 1) * KT : KT;

#if QS_FAST_PAIRS == 2
    static_assert(!CX && VEC && !EDGE, "the mirrored epilogue exists for the exact fp64 forms");
    int64_t b_mirror = 0;        // flat index j n + i of the pair that the last decode()'s pair (i, j) mirrors to
#elif QS_FAST_PAIRS == 4
    static_assert(QS_FAST_DMA && !CX && VEC && !EDGE && TN == 4, "the lower-from-mirror form exists for the exact fp64 DMA forms");
    int64_t b_mirror = 0;        // flat index j n + i of the pair whose blocks (J, G) are the last decode()'s pair's blocks (G, J < G)
#endif
    // The arguments as decode() reads them.  Column triangle: the fields that only a tile change needs (the tile grid, the
    // triangle's three) are read from the kernarg segment there, through a pointer the compiler cannot see through, and so
    // hold no scalar registers across the k-stages -- with them live the stage loop reloaded a spilled scalar in every stage.
#if QS_FAST_PAIRS == 3 && QS_FAST_STAGE_M0
    auto tile_args = [&]() {
        auto ka = (const __attribute__((address_space(4))) FastUpperArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        return ka;
    };
#else
    auto tile_args = [&]() { return &g; };
#endif
    // tile coordinates of virtual block v
    auto decode = [&](unsigned v, int& m0, int& n0, int64_t& b) {
        const auto* gd = tile_args();
        unsigned w = xcd_chunked_index_fast(v, gd->total);
        int mt, nt;
        if (gd->group_along_m) {
            mt = w % gd->tiles_m; w /= gd->tiles_m;
            nt = w % gd->tiles_n; w /= gd->tiles_n;
        } else {
            nt = w % gd->tiles_n; w /= gd->tiles_n;
            mt = w % gd->tiles_m; w /= gd->tiles_m;
        }
        // integer division runs on the vector ALU; bring the (wave-uniform) results back to
        // scalar registers so that every pointer derived from them stays an SGPR base
        b = __builtin_amdgcn_readfirstlane((int)w);
        // triangular batch: entry b is a pair (i, j >= i), its operands sit at the flat index i n + j
#if QS_FAST_PAIRS == 1
        b = (uint32_t)__builtin_amdgcn_readfirstlane((int)triangle_flat((uint32_t)b, gd->pairs));
#elif QS_FAST_PAIRS == 2 || QS_FAST_PAIRS == 4
        {
            const uint32_t pi = triangle_row((uint32_t)b, gd->pairs), pj = pi + ((uint32_t)b - triangle_row_start(pi, gd->pairs));
            b = (uint32_t)__builtin_amdgcn_readfirstlane((int)(pi * gd->pairs + pj));
            b_mirror = (uint32_t)__builtin_amdgcn_readfirstlane((int)(pj * gd->pairs + pi));
        }
#endif
        m0 = __builtin_amdgcn_readfirstlane(mt) * BM;
#if QS_FAST_PAIRS == 3
        {
            // n-tile -> (stack entry e, tile t of its side x side matrix).  S x S super-blocks hold S^2 / 128 tiles of R rows each
            // and form an upper triangle themselves: super-block sb is the pair (I, J >= I), the tile's first element (I S + sub R, J S).
            const uint32_t e = (uint32_t)nt / gd->per_matrix, t = (uint32_t)nt - e * gd->per_matrix;
            const uint32_t tshift = 2u * gd->sshift - 7u, sb = t >> tshift, sub = t & ((1u << tshift) - 1u);
            const uint32_t ns = gd->side >> gd->sshift;
            const uint32_t I = triangle_row(sb, ns), J = I + (sb - triangle_row_start(I, ns));
            n0 = __builtin_amdgcn_readfirstlane((int)((e * gd->side + (I << gd->sshift) + sub * (128u >> gd->sshift)) * gd->side + (J << gd->sshift)));
        }
#else
        n0 = __builtin_amdgcn_readfirstlane(nt) * BN;
#endif
    };

    // ---- fetch cursor: scalar bases of the tile being loaded + loop-invariant lane offsets
    // The bases are kept as scalar 64-bit integers and the loads go through buffer
    // descriptors built from them: a descriptor lives in SGPRs by construction, which pins
    // the scalar-base addressing even though the bases are re-aimed at every tile change.
    uint64_t a_ptr[NA];
    uint64_t b_ptr[NB];
    unsigned f_v = blockIdx.x;   // virtual block the cursor is in
    int f_k = 0;                 // next k-stage to load in that tile
    bool f_valid = true;
#if QS_FAST_PAIRS == 4
    // A wave-instruction i of this wave is one half (rows 8 (wave & 1) ...) of the 16-row group f_g + 2 i of the entry.  At the
    // k-stages f_k >= that group the block (group, f_k) is there and is fetched as ever (base a_nat + i RA rows, a_step per
    // stage); before, the mirror entry's block (f_k, group) lands as it is: its rows 16 f_k + 8 (wave & 1) ..., columns
    // 16 group ..., t_step = 16 rows per stage.  voff_a serves both (8 rows x 8 slots, row stride lda, and the wave's 8 wave rows,
    // which the turned base takes off again).
    uint64_t a_nat = 0;
    int f_g = 0;
    const size_t t_step = (size_t)16 * g.lda * 8;
#endif
    auto aim = [&](unsigned v) {
        int m0, n0; int64_t b;
        decode(v, m0, n0, b);
        const char* Ab = reinterpret_cast<const char*>(g.A + (b * g.sa + (int64_t)m0 * g.lda) * ES);
        const char* Bb = reinterpret_cast<const char*>(g.B + (b * g.sb + n0) * ES);
#if QS_FAST_PAIRS == 4
        a_nat = uniform64(reinterpret_cast<uint64_t>(Ab));
        f_g = (m0 >> 4) + (wave >> 1);
        const uint64_t a_turned = uniform64(reinterpret_cast<uint64_t>(g.A + b_mirror * g.sa) +
                                            (uint64_t)((int64_t)(8 * (wave & 1) - 8 * wave) * g.lda * 8));
#pragma unroll
        for (int i = 0; i < NA; ++i)
            a_ptr[i] = f_g + 2 * i > 0 ? a_turned + (uint64_t)(f_g + 2 * i) * 128u : a_nat + (uint64_t)i * RA * g.lda * ESZ;
#else
#pragma unroll
        for (int i = 0; i < NA; ++i) a_ptr[i] = uniform64(reinterpret_cast<uint64_t>(Ab + (size_t)i * RA * g.lda * ESZ));
#endif
        // B rows: the wave's first row of an item step is part of the scalar base (no limit on
        // ldb); only when a wave-instruction spans several rows (IPR_B < 64) does the lane
        // offset carry a row term
        const int brow0 = (wave * 64) / IPR_B;
#pragma unroll
        for (int i = 0; i < NB; ++i) b_ptr[i] = uniform64(reinterpret_cast<uint64_t>(Bb + (size_t)(brow0 + i * RPS) * g.ldb * ESZ));
    };
    aim(f_v);
    // (DMA form: the lane loads the k-pair whose swizzled slot is its lane-linear destination -- rows (tid / IPR_A) and
    // (tid / IPR_A) + i RA agree in bits 1-3, so the permutation is loop-invariant)
    const unsigned voff_a = (unsigned)(tid / IPR_A) * (unsigned)g.lda * (unsigned)ESZ +
                            (unsigned)(kDma ? (tid % IPR_A) ^ (((tid / IPR_A) >> 1) & 7) : tid % IPR_A) * IB;
#if QS_FAST_PAIRS == 3
    // column triangle: the tile's column 2 lane is column (2 lane) % S of segment (2 lane) / S, a row of the (c, d) matrix
    // apart -- one wave-instruction reads R pieces of 8 S bytes; its lane-linear destination is the B row as ever
    static_assert(kDma && TN == 4, "the column-triangle form exists for the exact fp64 DMA forms, 128 columns");
    const unsigned voff_b = (((2u * lane) >> g.sshift) * g.side + ((2u * lane) & ((1u << g.sshift) - 1u))) * (unsigned)ESZ;
#else
    const unsigned voff_b = (IPR_B < 64 ? (unsigned)(lane / IPR_B) * (unsigned)g.ldb * (unsigned)ESZ : 0u) +
                            (unsigned)(tid % IPR_B) * IB;
#endif
    const size_t a_step = KT * ESZ;
    const size_t b_step = (size_t)KT * g.ldb * ESZ;

    // ---- LDS addressing: one base per operand and direction, the rest immediates
    double* st_a = kSwizzleA ? As + (tid / IPR_A) * SA + ((tid % IPR_A) ^ (2 * (((tid / IPR_A) >> 2) & 3)))
                             : As + (tid / IPR_A) * SA + (tid % IPR_A) * DPI;
    double* st_b = Bs + (tid / IPR_B) * SB + (tid % IPR_B) * DPI;
    const double* rd_a = As + (wm * 16 * TM + (lane & 15)) * SA + (lane >> 4);
    // complex: the swizzled position of k = 4 kk + (lane >> 4) depends on kk -- one base per k-step of a stage (KS = 2)
    const int swz_r = kSwizzleA ? 2 * (((lane & 15) >> 2) & 3) : 0;
    const double* rd_a_cx[2] = {As + (wm * 16 * TM + (lane & 15)) * SA + ((lane >> 4) ^ swz_r),
                                As + (wm * 16 * TM + (lane & 15)) * SA + ((4 + (lane >> 4)) ^ swz_r)};
    // fp64: lane c of n-tile pair (2jp, 2jp+1) owns the ADJACENT columns 32jp + 2c, 32jp + 2c + 1,
    // so one 16-byte LDS read feeds two MFMA tiles and the epilogue stores 16 bytes per lane.  (Every such item is put
    // together from two accumulator blocks, four vector moves and a wait state per store, 124 + 31 per tile and wave: with two
    // waves per SIMD they cost nothing measurable, and a layout without them was slower -- profiles/gemm_fast_epilogue_ab.txt.)
    const double* rd_b = Bs + (lane >> 4) * SB + wn * 16 * TN + (CX ? 1 : 2) * (lane & 15);
    // DMA form: k = 4 kk + (lane >> 4) sits in slot (2 kk + (lane >> 5)) ^ ((row >> 1) & 7) of its row, an XOR with kk --
    // one offset per k-step of a stage (KS = 4) and, on top, per 16-row block i: the blocks are 2048 bytes apart, and
    // reads of one base at those distances are fused into ds_read2st64_b64, which banks over 32 banks instead of 64
    // (the even and odd rows of a half wave then collide: SQ_LDS_BANK_CONFLICT 1.1e9 per launch at l = 256).  An empty
    // asm makes each offset opaque, so no two fragment reads share a base (16 VGPRs, set once).
    // (lower-from-mirror form: its offsets change inside a tile, so the shift to bytes and the base could not be hoisted and
    // were a vector instruction per read: that form keeps whole LDS byte addresses)
    typedef const __attribute__((address_space(3))) double* lds_cdouble;
    constexpr unsigned RD_SC = (QS_FAST_PAIRS == 4 && QS_FAST_STAGE_M0) ? (unsigned)sizeof(double) : 1u;
    unsigned rd_a_dma[KS][TM];
    if constexpr (kDma) {
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                rd_a_dma[kk][i] = (unsigned)((wm * 16 * TM + i * 16 + (lane & 15)) * SA +
                                             2 * ((2 * kk + (lane >> 5)) ^ ((lane >> 1) & 7)) + ((lane >> 4) & 1)) * RD_SC;
                if constexpr (RD_SC != 1u) rd_a_dma[kk][i] += (unsigned)(uintptr_t)(lds_cdouble)As;
                asm volatile("" : "+v"(rd_a_dma[kk][i]));
            }
        }
    }
#if QS_FAST_PAIRS == 4
    // A turned block sits in LDS as [dd = d - 16 j][cc = c - 16 G]: lane (r = lane & 15, kq = lane >> 4) reads at k-step kk row
    // dd = 4 kk + kq, slot (r >> 1) ^ ((dd >> 1) & 7), double r & 1 -- the slot is the natural read's, so the two offsets differ
    // by 16 (4 kk + kq - r) + (r & 1) - (kq & 1), one lane value and 64 kk.  A half wave then reads two whole adjacent 128-byte
    // rows.  Row group i of the wave's rows (group c_g + i of the entry) is read turned at the k-stages c_k < c_g + i: the
    // offsets are rewritten at the tile's first stage and at the group's own, ahead of the first fragments of that stage.
    const unsigned rd_a_turn = (unsigned)(16 * ((lane >> 4) - (lane & 15)) + (lane & 1) - ((lane >> 4) & 1)) * RD_SC;
    auto turn = [&](int i, bool to_turned) __attribute__((always_inline)) {
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            if (to_turned) rd_a_dma[kk][i] += rd_a_turn + 64u * RD_SC * kk; else rd_a_dma[kk][i] -= rd_a_turn + 64u * RD_SC * kk;
            asm volatile("" : "+v"(rd_a_dma[kk][i]));
        }
    };
    int c_g = 0;                 // first 16-row group of this wave's rows in the tile being computed
    auto open_tile = [&](unsigned v) {
        int m0, n0; int64_t b;
        decode(v, m0, n0, b);
        c_g = (m0 >> 4) + wm * TM;
#pragma unroll
        for (int i = 0; i < TM; ++i)
            if (c_g + i > 0) turn(i, true);
    };
#endif
    // DMA destinations: the wave's first 16-byte item of each item step (lane-linear after it)
    double* dst_a = As + wave * DST_A_WAVE;
    double* dst_b = Bs + wave * DST_B_WAVE;

    // two staging register sets: the data of global stage s waits in set s & 1, so a load has
    // two stages (not one) to arrive from HBM before it is written to LDS
    item_t ra[2][NA], rb[2][NB];

    // load the cursor's stage into registers and advance the cursor (to the
    // next tile of this workgroup after the last k-stage)
    auto fetch = [&](auto set_c) {
        constexpr int set = decltype(set_c)::value;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            ra[set][i] = Item::load(a_ptr[i], EDGE ? bytes_left(g.a_end, a_ptr[i]) : 0xFFFFFFFFu, voff_a);
            a_ptr[i] += a_step;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            rb[set][i] = Item::load(b_ptr[i], EDGE ? bytes_left(g.b_end, b_ptr[i]) : 0xFFFFFFFFu, voff_b);
            b_ptr[i] += b_step;
        }
        if (++f_k == nk) {
            f_k = 0;
            f_v += P;
            f_valid = f_v < g.total;
            if (f_valid) aim(f_v);
        }
    };

    // DMA form: load the cursor's stage straight into LDS stage `buf` (one wave-instruction = 1 KB: eight A rows or one
    // B row) and advance the cursor.  The LDS base goes to M0 on the scalar ALU.
    static_assert(!kDma || (IPR_A == 8 && IPR_B == 64), "DMA staging: a wave-instruction is eight A rows or one B row");
    constexpr int NDMA = NA + NB;                       // DMA wave-instructions per stage
    auto fetch_dma = [&](auto buf_c) {
        constexpr int buf = decltype(buf_c)::value;
        typedef __attribute__((address_space(3))) void* lds_ptr;
#if QS_FAST_PAIRS != 0 && QS_FAST_STAGE_M0
        // The sixteen destinations (two buffers x NDMA) are loop-invariant sums: hoisted, they are sixteen scalars that the
        // overloads have no room for, and each came back through a v_readlane in every stage.  One opaque base per call
        // keeps them one scalar add each, and both bases come from the wave's number: dst_a and dst_b above, in bytes, from
        // the same constants.  (The plain batch has the room: its kernels stay as they were.)
        unsigned wave_o = (unsigned)wave;
        asm volatile("" : "+s"(wave_o));
        const unsigned lds_0 = (unsigned)(uintptr_t)(lds_ptr)smem;
        const unsigned lds_a = lds_0 + wave_o * (unsigned)(DST_A_WAVE * sizeof(double));
        const unsigned lds_b = lds_0 + (unsigned)(B_BASE * sizeof(double)) + wave_o * (unsigned)(DST_B_WAVE * sizeof(double));
#define QS_FAST_DST_A(off) ((lds_ptr)(uintptr_t)(lds_a + (unsigned)((off) * sizeof(double))))
#define QS_FAST_DST_B(off) ((lds_ptr)(uintptr_t)(lds_b + (unsigned)((off) * sizeof(double))))
#else
#define QS_FAST_DST_A(off) ((lds_ptr)(dst_a + (off)))
#define QS_FAST_DST_B(off) ((lds_ptr)(dst_b + (off)))
#endif
#pragma unroll
        for (int i = 0; i < NA; ++i) {
#if QS_FAST_PAIRS == 4
            // (the group's own stage: from here on its blocks are the entry's own)
            if (f_k == f_g + 2 * i) a_ptr[i] = a_nat + (uint64_t)i * RA * g.lda * ESZ + (uint64_t)f_k * a_step;
#endif
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(a_ptr[i]), (short)0, -1, 0x00020000);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, QS_FAST_DST_A(buf * A_STAGE + i * RA * SA), 16, (int)voff_a, 0, 0, 0);
#if QS_FAST_PAIRS == 4
            a_ptr[i] += f_k < f_g + 2 * i ? t_step : a_step;
#else
            a_ptr[i] += a_step;
#endif
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(b_ptr[i]), (short)0, -1, 0x00020000);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, QS_FAST_DST_B(buf * B_STAGE + i * RPS * SB), 16, (int)voff_b, 0, 0, 0);
            b_ptr[i] += b_step;
        }
#undef QS_FAST_DST_A
#undef QS_FAST_DST_B
        if (++f_k == nk) {
            f_k = 0;
            f_v += P;
            f_valid = f_v < g.total;
            if (f_valid) aim(f_v);
        }
    };

    int s_k = 0;   // k-stage (inside its tile) of the next stage to be written to LDS
    auto stash = [&](auto buf_c) {   // stage data of parity `buf` -> LDS stage `buf`
        constexpr int buf = decltype(buf_c)::value;
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (EDGE) {
            // last k-stage of a tile with a K tail: zero the k >= K part of both operands
            const bool tail = (s_k == nk - 1) && (k_tail < KT);
            if (++s_k == nk) s_k = 0;
            if (tail) {
                const item_t zero = item_t(0.0);
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    if constexpr (EPI == 2) {
                        if ((tid % IPR_A) * 2 >= k_tail) ra[buf][i][0] = 0.0;
                        if ((tid % IPR_A) * 2 + 1 >= k_tail) ra[buf][i][1] = 0.0;
                    } else {
                        if ((tid % IPR_A) >= k_tail) ra[buf][i] = zero;
                    }
                }
#pragma unroll
                for (int i = 0; i < NB; ++i)
                    if (tid / IPR_B + i * RPS >= k_tail) rb[buf][i] = zero;
            }
        }
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            double* d = st_a + buf * A_STAGE + i * RA * SA;
            if constexpr (CX) { d[0] = ra[buf][i][0]; d[BM * SA] = ra[buf][i][1]; }
            else if constexpr (VEC) *reinterpret_cast<f64x2*>(d) = ra[buf][i];
            else d[0] = ra[buf][i];
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            double* d = st_b + buf * B_STAGE + i * RPS * SB;
            if constexpr (CX) { d[0] = rb[buf][i][0]; d[KT * SB] = rb[buf][i][1]; }
            else if constexpr (VEC) *reinterpret_cast<f64x2*>(d) = rb[buf][i];
            else d[0] = rb[buf][i];
        }
    };

    f64x4 acc[NP][TM][TN];

    auto read_frags = [&](auto buf_c, int kk, double (&af)[NP][TM], double (&bf)[NP][TN]) {
        constexpr int buf = decltype(buf_c)::value;
        const double* as = (CX ? rd_a_cx[kk & 1] - kk * 4 : rd_a) + buf * A_STAGE;
        const double* bs = rd_b + buf * B_STAGE;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                if constexpr (kDma && RD_SC != 1u)
                    af[p][i] = *(lds_cdouble)(uintptr_t)(rd_a_dma[kk][i] + (unsigned)(buf * A_STAGE * sizeof(double)));
                else if constexpr (kDma) af[p][i] = As[rd_a_dma[kk][i] + buf * A_STAGE];
                else af[p][i] = as[p * BM * SA + i * 16 * SA + kk * 4];
            }
            if constexpr (CX) {
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[p][j] = bs[p * KT * SB + kk * 4 * SB + j * 16];
            } else {
#pragma unroll
                for (int jp = 0; jp < TN / 2; ++jp) {
                    const f64x2 v = *reinterpret_cast<const f64x2*>(bs + kk * 4 * SB + jp * 32);
                    bf[p][2 * jp] = v[0];
                    bf[p][2 * jp + 1] = v[1];
                }
            }
        }
    };
    // `fresh`: first k-step of a tile -- the accumulators start from C = 0
    auto mfma_step = [&](const double (&af)[NP][TM], const double (&bf)[NP][TN], auto fresh_c) {
        constexpr bool fresh = decltype(fresh_c)::value;
        const f64x4 zero = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if constexpr (!CX) {
                    acc[0][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[0][i], bf[0][j], fresh ? zero : acc[0][i][j], 0, 0, 0);
                } else {
                    acc[0][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[0][i], bf[0][j], fresh ? zero : acc[0][i][j], 0, 0, 0);
                    acc[1][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[0][i], bf[1][j], fresh ? zero : acc[1][i][j], 0, 0, 0);
                    acc[0][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-af[1][i], bf[1][j], acc[0][i][j], 0, 0, 0);
                    acc[1][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[1][i], bf[0][j], acc[1][i][j], 0, 0, 0);
                }
            }
        }
    };

    // epilogue of the tile at virtual block v: reg r of a lane -> row (lane>>4) + 4r of
    // each 16-row block; 16 bytes per lane (8-byte pieces in the !VEC form).  `guard`:
    // border tile of the edge form, rows >= m and columns >= n are not stored.
#if QS_FAST_PAIRS == 2
    bool mirrored = false;       // the last epilogue stored its tile twice (wave-uniform)
#endif
    auto epilogue = [&](unsigned v) __attribute__((always_inline)) {
        int m0, n0; int64_t b;
        decode(v, m0, n0, b);
        const int64_t row_l = (int64_t)m0 + wm * 16 * TM + (lane >> 4);
#if QS_FAST_PAIRS == 3
        // column triangle: tile column wn 64 + jp 32 + 2 (lane & 15) in segments of S -- the lane's own part, and jp steps
        // 32 / S rows of the (c, d) matrix (16 bytes per lane still; eight lanes complete a 128-byte line)
        const unsigned tcl = (unsigned)(wn * 16 * TN + 2 * (lane & 15));
        const int col_l = n0 + (int)((tcl >> g.sshift) * g.side + (tcl & ((1u << g.sshift) - 1u)));
        const int64_t jp_step = (int64_t)((32u >> g.sshift) * g.side);
#else
        const int col_l = n0 + wn * 16 * TN + (CX ? 1 : 2) * (lane & 15);
        constexpr int jp_step = 32;
#endif
        double* __restrict__ C = g.C + (b * g.sc + row_l * g.ldc + col_l) * ES;
        auto store_all = [&](auto add_c, auto guard_c) __attribute__((always_inline)) {
            constexpr bool add = decltype(add_c)::value;
            constexpr bool guard = decltype(guard_c)::value;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double* crow = C + (int64_t)(i * 16 + 4 * r) * g.ldc * ES;
                    const bool row_ok = !guard || row_l + i * 16 + 4 * r < g.m;
                    if constexpr (CX) {
#pragma unroll
                        for (int j = 0; j < TN; ++j) {
                            if (row_ok && (!guard || col_l + j * 16 < g.n)) {
                                f64x2* dst = reinterpret_cast<f64x2*>(crow + 2 * j * 16);
                                f64x2 v2 = f64x2{acc[0][i][j][r], acc[1][i][j][r]};
                                if constexpr (add) v2 += *dst;
                                QS_FAST_STORE(dst, v2);
                            }
                        }
                    } else if constexpr (VEC) {
#pragma unroll
                        for (int jp = 0; jp < TN / 2; ++jp) {
                            if (row_ok && (!guard || col_l + jp * 32 + 1 < g.n)) {
                                f64x2* dst = reinterpret_cast<f64x2*>(crow + jp * jp_step);
#if QS_FAST_ABLATE_EPI_COPIES
                                // (measurement only: the item is half of ONE accumulator block, registers as they lie)
                                f64x2 v2 = kDma ? f64x2{acc[0][i][2 * jp + (r >> 1)][2 * (r & 1)], acc[0][i][2 * jp + (r >> 1)][2 * (r & 1) + 1]}
                                                : f64x2{acc[0][i][2 * jp][r], acc[0][i][2 * jp + 1][r]};
#else
                                f64x2 v2 = f64x2{acc[0][i][2 * jp][r], acc[0][i][2 * jp + 1][r]};
#endif
                                if constexpr (add) v2 += *dst;
                                QS_FAST_STORE(dst, v2);
                            } else if (guard && row_ok && col_l + jp * 32 < g.n) {   // odd n: the last column alone
                                double* dst = crow + jp * 32;
                                double v1 = acc[0][i][2 * jp][r];
                                if constexpr (add) v1 += *dst;
                                *dst = v1;
                            }
                        }
                    } else {
#pragma unroll
                        for (int jp = 0; jp < TN / 2; ++jp) {
#pragma unroll
                            for (int h = 0; h < 2; ++h) {
                                if (row_ok && (!guard || col_l + jp * 32 + h < g.n)) {
                                    double* dst = crow + jp * 32 + h;
                                    double v1 = acc[0][i][2 * jp + h][r];
                                    if constexpr (add) v1 += *dst;
                                    *dst = v1;
                                }
                            }
                        }
                    }
                }
            }
        };
        const bool border = EDGE && ((int64_t)m0 + BM > g.m || n0 + BN > g.n);   // wave-uniform
        if (border) {
            if constexpr (EDGE) {
                if (g.accumulate) store_all(std::true_type{}, std::true_type{});
                else store_all(std::false_type{}, std::true_type{});
            }
        } else {
            if (g.accumulate) store_all(std::true_type{}, std::false_type{});
            else store_all(std::false_type{}, std::false_type{});
        }
#if QS_FAST_PAIRS == 2
        // The mirror: entry (row, col) of pair (i, j > i) also goes to (col, row) of pair (j, i), which no tile of the launch
        // reads or writes (m == n, no accumulate: the host checks).  A lane holds rows (lane >> 4) + 4 r + 16 i and two
        // adjacent columns, so one 8-byte store at fixed (i, jp, h, r) writes 16 runs of 32 bytes -- the four lane groups are
        // four consecutive transposed columns -- and the four r, issued back to back, complete 16 whole 128-byte lines.  The
        // column offsets are wave-uniform; the skip of a diagonal pair is a scalar branch.
        mirrored = b_mirror != b;
        if (mirrored) {
            double* __restrict__ T = g.C + b_mirror * g.sc + (int64_t)col_l * g.ldc + row_l;
#pragma unroll
            for (int jp = 0; jp < TN / 2; ++jp) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    double* tcol = T + (int64_t)(jp * 32 + h) * g.ldc;
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) QS_FAST_STORE(tcol + i * 16 + 4 * r, acc[0][i][2 * jp + h][r]);
                    }
                }
            }
        }
#endif
    };

    using B0 = std::integral_constant<int, 0>;
    using B1 = std::integral_constant<int, 1>;
    using T_ = std::true_type;
    using F_ = std::false_type;

    // number of tiles of this workgroup and of global stages
    const unsigned my_tiles = (g.total - blockIdx.x + P - 1) / P;
    const int64_t stages = (int64_t)my_tiles * nk;

    double a0[NP][TM], b0[NP][TN], a1[NP][TM], b1[NP][TN];
    if constexpr (kDma) {
        fetch_dma(B0{});               // global stage 0
        if (f_valid) {
            fetch_dma(B1{});           // stage 1
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NDMA) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    } else {
        fetch(B0{});                   // global stage 0
        stash(B0{});
        __syncthreads();
        if (f_valid) fetch(B1{});      // stage 1
        if (f_valid) fetch(B0{});      // stage 2
    }
#if QS_FAST_PAIRS == 4
    open_tile(blockIdx.x);
#endif
    read_frags(B0{}, 0, a0, b0);

    unsigned c_v = blockIdx.x;   // virtual block being computed
    int c_k = 0;                 // its current k-stage
    bool after_epi = false;      // DMA form: the previous stage ended with an epilogue
    constexpr int EPI_ST = TM * 4 * (TN / 2);   // its stores per wave (VEC form)
    static_assert(EPI_ST < 64, "the vmcnt field holds 0..63");
#if QS_FAST_PAIRS == 2
    // A mirrored epilogue issues EPI_ST + TM * 4 * TN stores, more than the field counts: the wait below then asks for at
    // most 63 operations in flight, which is the DMA (older than every store) and the oldest EPI_ST + TM * 4 * TN - 63 stores.
    static_assert(EPI_ST + TM * 4 * TN > 63, "otherwise count the mirror stores exactly");
#endif

    // one global stage: k-steps 0 .. KS-2, [stash the next stage], barrier, [fetch the
    // stage after next], [first fragments of the next stage], k-step KS-1, and at a tile's
    // last k-stage its epilogue.  All conditions are wave-uniform (scalar branches).
    auto stage = [&](auto cur_c, int64_t gs) {
        constexpr int cur = decltype(cur_c)::value;
        using NXT = std::integral_constant<int, cur ^ 1>;
        const bool has_next = gs + 1 < stages;
        // Edge form, last k-stage of a tile: its k-steps beyond K multiply zeros -- they are skipped (wave-uniform branches
        // around the MFMAs only: K = 130 walks 33 k-steps instead of 36, K = 66 17 instead of 20).  Adding 0 . 0 never
        // changed a value, so results stay bit-identical to the kernels that do not skip.
        const int ks_live = (EDGE && c_k == nk - 1) ? (k_tail + 3) / 4 : KS;
        // k-step 0 (fresh accumulators at the start of a tile)
        read_frags(cur_c, 1, a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        if (c_k == 0) mfma_step(a0, b0, T_{}); else mfma_step(a0, b0, F_{});
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 1; kk + 1 < KS; ++kk) {
            if ((kk & 1) == 0) { read_frags(cur_c, kk + 1, a1, b1); __builtin_amdgcn_sched_barrier(0); if (!EDGE || kk < ks_live) mfma_step(a0, b0, F_{}); }
            else               { read_frags(cur_c, kk + 1, a0, b0); __builtin_amdgcn_sched_barrier(0); if (!EDGE || kk < ks_live) mfma_step(a1, b1, F_{}); }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (kDma) {
            // Stage gs+1 has landed in LDS buffer NXT once its DMA, issued after the previous barrier, is done: the only
            // vector-memory work issued since is the previous stage's epilogue (EPI_ST stores), which is not waited for.
            // lgkmcnt(0): this wave's fragment reads of buffer `cur` are done before anyone's DMA overwrites it.  A raw
            // s_barrier, because __syncthreads() would also wait for the DMA of the stage after.
#if QS_FAST_PAIRS == 2
            if (after_epi && mirrored) asm volatile("s_waitcnt vmcnt(63) lgkmcnt(0)" ::: "memory");
            else
#endif
            if (after_epi) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"i"(EPI_ST) : "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            after_epi = false;
            if (f_valid) fetch_dma(cur_c);     // stage gs+2 into the buffer just read
            __builtin_amdgcn_sched_barrier(0);
        } else {
            if (has_next) stash(NXT{});        // stage gs+1, loaded two stages ago
            __syncthreads();
            if (f_valid) fetch(NXT{});         // stage gs+3 into the set just written out
        }
#if QS_FAST_PAIRS == 4
        // (every fragment read of this stage has been issued: the offsets may go over to the next stage's)
        if (has_next) {
            if (c_k + 1 == nk) {
                open_tile(c_v + P);
            } else {
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    if (c_k + 1 == c_g + i) turn(i, false);
            }
        }
#endif
        if (has_next) read_frags(NXT{}, 0, a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        if (!EDGE || KS - 1 < ks_live) mfma_step(a1, b1, F_{});
        __builtin_amdgcn_sched_barrier(0);
        if (++c_k == nk) {
            epilogue(c_v);
            c_k = 0;
            c_v += P;
            after_epi = true;
        }
    };

    for (int64_t gs = 0; gs < stages; gs += 2) {
        stage(B0{}, gs);
        if (gs + 1 < stages) stage(B1{}, gs + 1);
    }
