// fr_coop_kernel_body.inc - the body of fr_coop_kernel and fr_coop_lp_kernel (fr_coop.hip), which
// differ in the objective alone: LP (a constexpr bool of the including kernel) selects the kinematic
// link-position model's; WR (likewise) the simulated end-effector
// wrench in the rows' step (coop_rows).  Text shared by inclusion, so the default mode's kernels compile from the
// very statements they always had.
    constexpr int KS = EN ? LDS_KIN_EN : LDS_KIN;
    __shared__ __attribute__((aligned(16))) double lds_kin[WPB * ROWS_PER_WAVE * KS];
    __shared__ __attribute__((aligned(16))) double lds_scr[WPB * ROWS_PER_WAVE * LDS_SCR];
    __shared__ double Lmodel[LDS_MODEL];
    __shared__ double Lx0[MAX_X];
    if (a.optimal && (a.status->all_nan || a.status->sg_error)) return;   // no filter() (mppi.cpp:170-176)
    const int wv = (WPB == 1) ? 0 : (int)(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int rowi = lane >> 4;
    const int wrow = wv * ROWS_PER_WAVE + rowi;   // row within the workgroup
    const int wblk = blockIdx.x * WPB + wv;        // wave index in the launch
    int rk = 0x7FFFFFFF;
    if constexpr (WPB == 4) rk = kept_rank(a, (int64_t)wblk * ROWS_PER_WAVE + rowi);
    stage_body_table(a, Lmodel, 64 * WPB);
    stage_x0(a, Lx0);
    __syncthreads();
    if constexpr (WPB == 4) {
        if (a.drawn_ahead) {
            if (blockIdx.x == 0 && wv == 1) block0_sample_writes<64>(a, lane);
            kept_rows_wave(a, (int64_t)wblk * ROWS_PER_WAVE + rowi, lane, rk);
        }
    }
    coop_rows<CK, EN, false, 0, false, KC, WR>(a, (int64_t)wblk * ROWS_PER_WAVE + rowi, lane, wblk, lds_kin + wrow * KS,
                                               lds_scr + wrow * LDS_SCR, Lmodel, Lx0);
    if constexpr (WPB == 4) {
        if (a.costs_in_launch) launch_costs<CK, EN, KC, LP>(a, wv, lane, Lmodel);
    } else if constexpr (WPB == 1) {
        // past one round (two waves per SIMD, several rounds): the wave's own rows' objective after
        // its loop, while the launch's other waves still run, instead of fr_step_cost_kernel after it
        if (a.costs_in_launch) {
            __builtin_amdgcn_s_waitcnt(0);   // the wave's own record stores, read back by other lanes
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
#pragma unroll 1
            for (int i = 0; i < ROWS_PER_WAVE; i++)
                launch_row_cost<CK, EN, KC, LP>(a, (int64_t)blockIdx.x * ROWS_PER_WAVE + i, lane, Lmodel);
        }
    }
