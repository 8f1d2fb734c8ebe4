// fr_coop_x_kernel_body.inc - the body of fr_coop_x_kernel and fr_coop_x_lp_kernel (fr_coop.hip);
// LP (a constexpr bool of the including kernel): the kinematic link-position model's objective;
// WR (likewise): the simulated end-effector wrench in the rows' step (coop_rows).
    constexpr int KS = EN ? LDS_KIN_EN : LDS_KIN;
    __shared__ __attribute__((aligned(16))) double lds_kin[5 * ROWS_PER_WAVE * KS];
    __shared__ __attribute__((aligned(16))) double lds_scr[5 * ROWS_PER_WAVE * LDS_SCR];
    __shared__ double Lmodel[LDS_MODEL];
    __shared__ double Lx0[MAX_X];
    __shared__ int Lflag[LF_N];      // records stored (main waves, relay), kept columns copied
    __shared__ int Lq[Q_N];          // the main waves' steps, chunk counters, the relay's stage
    __shared__ double Lst[64 * 3];   // the relay's (q, qd, E) per lane between stages
    __shared__ __attribute__((aligned(16))) double Lcs[5 * ROWS_PER_WAVE * HC_MAX];   // step costs of the groups' rows
    const int wv = (int)(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int rowi = lane >> 4;
    const int member = relay_member(a);   // of the relay rows this workgroup carries (-1: none)
    const bool xr = member >= 0;
    const int64_t lr = wv < 4 ? (int64_t)(blockIdx.x * 4 + wv) * ROWS_PER_WAVE + rowi
                              : a.xbase + (int64_t)((int)blockIdx.x % RELAY_STRIDE) * ROWS_PER_WAVE + rowi;   // (waves < 5)
    const int rk = (wv < 4 || (wv == 4 && xr)) ? kept_rank(a, lr) : 0x7FFFFFFF;
    stage_body_table(a, Lmodel, 64 * XW);
    stage_x0(a, Lx0);
    if (threadIdx.x < LF_N) Lflag[threadIdx.x] = 0;
    if (threadIdx.x < Q_N) Lq[threadIdx.x] = threadIdx.x < Q_NEXT ? -1 : 0;
    const int ng = xr ? 5 : 4;   // row groups of the objective
    if (threadIdx.x == Q_NEXT + 4) {   // the relay group's first chunk here (none: past every chunk)
        int cb, ce;
        group_chunks(a, 4, cb, ce);
        Lq[Q_NEXT + 4] = xr ? cb : 0x7FFF;
    }
    __syncthreads();
    // main wave w's rows use slots 4 w + i, the relay's rows (whichever wave runs them) 16 + i
    const int slot = wv < 4 ? wv * ROWS_PER_WAVE + rowi : 4 * ROWS_PER_WAVE + rowi;
    double *Lk = lds_kin + slot * KS, *Lw = lds_scr + slot * LDS_SCR;
    if (a.drawn_ahead) {
        if (blockIdx.x == 0 && wv == 1) block0_sample_writes<64>(a, lane);   // off the SIMD of the relay's first stage
        if (wv < 4) kept_rows_wave(a, lr, lane, rk);
        else if (wv == 4 && xr) {   // the relay rows' columns of the steps this member runs
            kept_rows_wave(a, lr, lane, rk, relay_member_step(a, member, a.H),
                           member + 1 < a.relay_k ? relay_member_step(a, member + 1, a.H) : 0x7FFFFFFF);
            __hip_atomic_store(Lflag + LF_KEPT_X, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    const bool cil = a.costs_in_launch != 0;
    // AssistedManipulation without the energy tank (STAGE_AHEAD, fr_coop.hip): a later relay member's
    // stage waves take objective chunks ahead of their stage.  The objective's chunks then have two
    // call sites (cost_work; each is a copy of the objective's code, and the kernel has to stay inside
    // the 64-KB instruction cache, fr_coop.hip cost_chunk): those waves ahead of their stage, and every
    // wave after its rows.  The tank's and TrackPoint's kernels keep a site per branch and no work
    // ahead: joined, their relay step loops grew (TrackPoint's from 776 to 821 instructions).
    if (wv < 4) {
        if (cil) {   // the next draws for this wave's rows may now overwrite their previous eps
            __builtin_amdgcn_s_waitcnt(0);
            __hip_atomic_store(Lflag + LF_KEPT + wv, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            __builtin_amdgcn_s_setprio(1);   // above the objective's waves, below the relay
        }
        const int wblk = blockIdx.x * 4 + wv;
        coop_rows<CK, EN, false, 0, true, false, WR>(a, (int64_t)wblk * ROWS_PER_WAVE + rowi, lane, wblk, Lk, Lw, Lmodel, Lx0,
                                                     nullptr, 0, 0x7FFFFFFF, Lq + Q_PROG + wv);
        __builtin_amdgcn_s_setprio(0);
        if (cil) {
            signal_records(Lflag + wv);
            if constexpr (!STAGE_AHEAD<CK, EN>) cost_work<CK, EN, LP>(a, wv, ng, lane, Lmodel, Lcs, Lflag, Lq);
        }
    } else {
        const int s = wv - 4;   // this wave's SIMD
        const bool relay = xr && (s == 0 || a.handover);
        if constexpr (STAGE_AHEAD<CK, EN>) {
            // Stages 1 .. 3 of a later member wait 80-115 us of the launch for their turn.  Their
            // workgroup's main waves store records all that time, and with nobody to evaluate them the
            // member's host began its closing with ten passes in hand and ended 15 us after every
            // other workgroup (profiles/launch_tail/).  These waves make their draws, take objective
            // chunks until the stage before their own runs (cost_work's `until`), then run their stage.
            const bool ahead = relay && cil && a.handover && a.stage_work && member > 0 && s > 0;
            if (ahead) {
                if (a.ahead_noise) group_draws(a, s, lane, Lflag);
                cost_work<CK, EN, LP>(a, s, ng, lane, Lmodel, Lcs, Lflag, Lq, s);
            }
            if (relay) relay_stage<CK, EN, WR>(a, s, member, lane, Lk, Lw, Lmodel, Lx0, Lflag, Lq, Lst, ahead);
        } else {
            if (relay) relay_stage<CK, EN, WR>(a, s, member, lane, Lk, Lw, Lmodel, Lx0, Lflag, Lq, Lst);
        }
        if (!cil) return;
        // the draws for main wave s's rows (relay stages made theirs before their stage; wave 0's
        // rows of a workgroup with rows left over are left to rank_draw_kernel)
        if (a.ahead_noise && !relay && !(member == 0 && s == 0)) group_draws(a, s, lane, Lflag);
        if constexpr (!STAGE_AHEAD<CK, EN>) cost_work<CK, EN, LP>(a, s, ng, lane, Lmodel, Lcs, Lflag, Lq);
    }
    if constexpr (STAGE_AHEAD<CK, EN>) {
        if (cil) {
            // (the lane opaque: what cost_work derives from it is otherwise formed ahead of the branches
            // and lives across the step loops)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            cost_work<CK, EN, LP>(a, wv & 3, ng, ln, Lmodel, Lcs, Lflag, Lq);
        }
    }
#ifdef COST_TRACE   // COOP_TRACE builds: slot 3 = the main wave's end (after its objective work); the traced
                    // relay hosts (cost_work): the ends of waves 4 .. 7
    if (a.trace && lane == 0 && wv < 4) a.trace[4 * (blockIdx.x * 4 + wv) + 3] = (uint32_t)__builtin_amdgcn_s_memrealtime();
    if (a.trace && wv >= 4 && xr && lane == 0 && (int)blockIdx.x % RELAY_STRIDE == 0 && (member == 0 || member == a.relay_k - 1))
        a.trace[4 * (gridDim.x * 4 + TR_HOSTS + (member == 0 ? 0 : 1) * TR_HOST_N + 41) + (wv - 4)] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif

