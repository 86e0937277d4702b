// The one-tile persistent stack walker, written ONCE: h2_phase.hpp includes this file three times, each time with
//   H2_WALK_KERNEL = the kernel's name, H2_WALK_FORM = 0 whole tiles with the cross-phase W prefetch (h2_stack_kernel),
//                                                    1 row-narrow ring (h2_stackn_kernel), 2 direct-W (h2_stackd_kernel)
// (the comments above the three includes say why each form exists; both names are undefined again at the end of this file).  The
// sharing is textual on purpose: between the __global__ entry and h2_phase there is no function and no lambda that the three kernels
// did not have when each was written out -- every inline level added OR removed there changed their gfx950 code (HISTORY.md) -- and
// what the forms do differently is selected by the constant FORM.
template <int NP>
__global__ __launch_bounds__(512, 2) void H2_WALK_KERNEL(const H2StackArgs s) {
    constexpr int FORM = H2_WALK_FORM;
    constexpr bool DW = FORM == 2;
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int tid = threadIdx.x;
    const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = s.G, D = s.D;
    int team, tn;
    {
        const int b = blockIdx.x;
        team = (b & 7) + 8 * ((b >> 3) / G);
        tn = (b >> 3) % G;
        if (team >= s.n_teams) return;
    }
    if (tid == 0) *reinterpret_cast<volatile unsigned*>(smem + H2_FAIL) = 0u;
    h2_publish_xcd(s, team, tid);
    int plain = 0, seen = 0;       // plain hand-off stores once the team is known to sit on one XCD (h2_publish_xcd)
    __syncthreads();
    [[maybe_unused]] H2Pf pf{0u, 0, nullptr, 0u, 1};      // form 0, cross-phase W prefetch: the first phase of the launch fills its own ring
    // a unit = what a team walks through every phase: a row tile (form 0), a sub-tile of s.rgs row groups (1), one row group (2)
    const int rs = FORM == 0 ? 1 : (FORM == 1 ? 4 / s.rgs : 4);      // units per row tile
    const int n_units = s.n_tiles * rs;
    for (int unit0 = team; unit0 < n_units; unit0 += s.n_teams) {
        unsigned need = 0;
        for (int ph = 0; ph < s.n_phases; ++ph, need += G) {
            if (!seen && ph >= 2) {       // the proj phase has seen every partner arrive: the team's placement word is complete
                plain = __builtin_amdgcn_readfirstlane(h2_team_on_one_xcd(s, team));
                seen = 1;
            }
            // the thread id is rebuilt from the wave index (a scalar) and the lane number every phase: kept in a register
            // across the phases it was the one value the 256-register budget spilled to scratch
            int wvp = wave_s, unit = unit0, tnp = tn;
            asm volatile("" : "+s"(wvp), "+s"(unit), "+s"(tnp));
            int tidp = wvp * 64 + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            asm volatile("" : "+v"(tidp));
            const int wv = wvp;
            // the unit's row tile, its first row group, the row groups a workgroup owns, and which waves multiply (h2_phase ACT; the
            // direct-W form: wave rg_lo and wave 4 + (rg_lo + 2) % 4, on different SIMDs)
            int tile = unit, rg_lo = 0, rgs = 4;
            [[maybe_unused]] bool act = true;
            if constexpr (FORM == 1) {
                tile = unit / rs;
                rg_lo = (unit - tile * rs) * s.rgs;
                rgs = s.rgs;
                act = (wv & 3) >= rg_lo && (wv & 3) < rg_lo + s.rgs;
            } else if constexpr (FORM == 2) {
                tile = unit >> 2;
                rg_lo = unit & 3;
                rgs = 1;
                act = wv < 4 ? wv == rg_lo : (wv & 3) == ((rg_lo + 2) & 3);
            }
            // one arrival counter per row tile (form 0: the first n_tiles words) or per sub-tile (H2_CTR_PER_TILE words per tile)
            unsigned* ctr = FORM == 0 ? s.counters + tile : s.counters + H2_CTR_PER_TILE * tile + rg_lo;
            const char* const* w = s.w[ph >> 2];
            bool ok = true;
            if (s.inject > 0 && ph == s.inject && unit == 0 && tnp == 0) return;     // fault injection (test hook)
            if constexpr (FORM == 0) {
                // the W stream the phase behind this one starts with (H2Pf): the next phase of this tile, or the first phase of the
                // team's next tile; nothing behind the last phase of the launch
                int nph = ph + 1;
                if (nph == s.n_phases) nph = unit0 + s.n_teams < s.n_tiles ? 0 : -1;
                pf.nw = nullptr;
                if (nph >= 0) {
                    const int kind = nph & 3;
                    const int npass = kind == 0 ? 3 : (kind == 2 ? 2 : 1);
                    const int ktn = h2_ksteps(kind == 3 ? 2 * D : D, NP);
                    if (npass * ktn >= H2_PF_MIN_T) {
                        // column group of pass g: g G + tn (qkv), 2 tn + g (fc1), tn (proj, fc2) -- h2_phase's colbase / BN
                        pf.nw = s.w[nph >> 2][kind] + (size_t)(npass == 3 ? tnp : npass * tnp) * ktn * H2_W;
                        pf.pstride = (unsigned)((npass == 3 ? G : 1) * ktn * H2_W);
                        pf.npass = npass;
                    }
                }
            }
// one role of a phase: form 0 whole tiles, entered prefetched (PF); forms 1, 2 the multiplying waves or the loader-only ones
#define H2_WALK_PHASE(NTW, WC, SLOT0, EPI, LNF, NPASS)                                                                                         \
    if constexpr (FORM == 0)                                                                                                                    \
        ok = h2_phase_pf<EPI, LNF, NPASS, NTW, WC, NP>(a, smem, tidp, wv, SLOT0, tile, tnp, ctr, need, pf);  \
    else                                                                                                                                        \
        ok = act ? h2_phase<EPI, LNF, NPASS, NTW, true, WC, 1, NP, true, DW>(a, smem, tidp, wv, SLOT0, tile, tnp, ctr, need, true, rg_lo, rgs)   \
                 : h2_phase<EPI, LNF, NPASS, NTW, true, WC, 1, NP, false, DW>(a, smem, tidp, wv, SLOT0, tile, tnp, ctr, need, true, rg_lo, rgs)
            switch (ph & 3) {
                case 0: {   // x = x + proj(attn(qkv(norm1(x))))   (Block.forward :84-90)
                    H2Args a = h2_args_qkv<NP>(s, w[0], D, G, plain);
                    H2_BY_ROLE(wv, DW, H2_WC, H2_WALK_PHASE, H2_EPI_ATT, true, 3);
                    break;
                }
                case 2: {   // x = x + fc2(gelu(fc1(norm2(x))))    (Block.forward :91, Mlp.forward :31-37)
                    H2Args a = h2_args_fc1<NP>(s, w[2], D, G, plain);
                    H2_BY_ROLE(wv, DW, H2_WC, H2_WALK_PHASE, H2_EPI_GELU, true, 2);
                    break;
                }
                default: {
                    const bool fc2 = (ph & 3) == 3;
                    H2Args a = h2_args_res<NP>(s, fc2 ? w[3] : w[1], fc2, D, G, plain);
                    H2_BY_ROLE(wv, DW, H2_WC, H2_WALK_PHASE, H2_EPI_RES, false, 1);
                    break;
                }
            }
#undef H2_WALK_PHASE
            if (!ok) return;
        }
    }
}
#undef H2_WALK_KERNEL
#undef H2_WALK_FORM
