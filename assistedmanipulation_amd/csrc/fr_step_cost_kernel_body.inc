// fr_step_cost_kernel_body.inc - the body of fr_step_cost_kernel and fr_step_cost_links_kernel
// (fr_cost.hip); LP (a constexpr bool of the including kernel): the kinematic link-position model;
// OB (with LP, the links kernel's template parameter): the obstacle term behind it, OB_TERM_NONE ..
// OB_TERM_HELD_SELF.
    __shared__ double Lj[FR_NB * JT_STRIDE];
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    const bool frow = a.fcost != nullptr && row == a.count;
    // no filter() when the update threw (mppi.cpp:170-176)
    if ((frow || a.optimal) && (a.status->all_nan || a.status->sg_error)) return;
    const int H = a.H;
    const StepConst *stp = frow ? a.fsteps : a.steps;
    const DevCost &Cs = *a.cost;
    if (CK != CK_TRACK_POINT)   // per-joint parameters (84 of them for 64 lanes)
        for (int i = lane; i < FR_NB * JT_STRIDE; i += 64) {
            const int j = i / JT_STRIDE, f = i - j * JT_STRIDE;
            const double *src = f < 3 ? &Cs.lower[j].bound + f : (f < 6 ? &Cs.upper[j].bound + (f - 3) : &Cs.vel_q[j]);
            Lj[i] = *src;
        }
    __syncthreads();
    const double J = rollout_cost<CK, EN, JT_STRIDE, KC, LP, OB>(Cs, stp, frow ? a.frec : a.rec + row * H * (KC ? FR_REC_C : FR_REC), H,
                                                             lane, Lj, LinkModel{a.model, a.dt});
    if (lane != 0) return;
    if (frow) *a.fcost = J;
    else if (a.optimal) *a.cost_out = J;
    else {
        a.cost_out[a.begin + row] = J;
        fold_cost_stats(a.stats, J, row);   // exact min / max / count, any order
    }
