// body of BeelerReuter::body<P, MODE, T> (T = float, or vf<R> for R cells at once) — included by models.hpp
        const T C = s[1], M = s[2], H = s[3], J = s[4], D = s[5], F = s[6], XI = s[7];
        // n = number of dt the slow gates advance (br.py:98-107): 1, or with skip 5 / 0
        // (k.skip == 2: solve(state, 0) on its own — the slow gates are held, FIBHIP_HOLD)
        // (`skip` as a compile-time constant: 82 v_mov, 15 branches and 24 scalar spills fewer, no time gained — 15.16 against
        // 15.11 us per tick; profiles/r04_ab_boundary_and_br.txt)
        const bool slow = k.skip == 2 ? false : (k.skip ? (sub == 0) : true);
        const float mdtn = k.skip ? k.mdt_skip : k.mdt;
        T M1, H1, J1 = J, D1 = D, F1 = F, XI1 = XI;
        if (MODE == MODE_CHEBY) {                                   // br.py:207-252
            constexpr float xmid = FC(0.5 * (30.0 + -90.0)), xhalf = FC(0.5 * (30.0 - -90.0));
            T S[9];
#ifdef FIB_BR_TABLE_INC
            constexpr const float *TBL = FIB_BR_CHEB;          // the table baked in as literals (specialised build)
#else
            const float *TBL = k.cheb;
#endif
            // always the correctly rounded quotient: the degree-8 sums amplify an ulp of x by ~1e2
            const T x = Exact::divc(V0 - xmid, xhalf, 1.0f / xhalf);           // :215
            S[0] = T_of<T>(1.0f); S[1] = x;                                  // calc_chebyshev_leading :289-301
#pragma unroll
            for (int i = 2; i <= 8; ++i) S[i] = (2.0f * x) * S[i - 1];
            M1 = rush_larsen<P>(M, cheb<P>(TBL + 0 * 9, S), cheb<P>(TBL + 2 * 9, S), k.mdt);
            H1 = rush_larsen<P>(H, cheb<P>(TBL + 1 * 9, S), cheb<P>(TBL + 3 * 9, S), k.mdt);
            if (slow) {
                XI1 = rush_larsen<P>(XI, cheb<P>(TBL + 4 * 9, S), cheb<P>(TBL + 8 * 9, S), mdtn);
                J1 = rush_larsen<P>(J, cheb<P>(TBL + 5 * 9, S), cheb<P>(TBL + 9 * 9, S), mdtn);
                D1 = rush_larsen<P>(D, cheb<P>(TBL + 6 * 9, S), cheb<P>(TBL + 10 * 9, S), mdtn);
                F1 = rush_larsen<P>(F, cheb<P>(TBL + 7 * 9, S), cheb<P>(TBL + 11 * 9, S), mdtn);
            }
        } else {                                                    // br.py:175-205
            T inf, tau;
            inf_tau<P>(ab<P>(V0, FC(0.0000f), FC(0.0f), FC(47.f), FC(-1.0f), FC(47.f), FC(-0.1f), FC(-1.0f)),
                       ab<P>(V0, FC(40.f), FC(-0.056f), FC(72.f), 0.0f, 0.0f, 0.0f, 0.0f), inf, tau);
            M1 = rush_larsen<P>(M, inf, tau, k.mdt);
            inf_tau<P>(ab<P>(V0, FC(0.126f), FC(-.25f), FC(77.f), 0.0f, 0.0f, 0.0f, 0.0f),
                       ab<P>(V0, FC(1.7f), FC(0.0f), FC(22.5f), 0.0f, 0.0f, FC(-0.082f), FC(1.0f)), inf, tau);
            H1 = rush_larsen<P>(H, inf, tau, k.mdt);
            if (slow) {
                inf_tau<P>(ab<P>(V0, FC(0.0005f), FC(0.083f), FC(50.f), 0.0f, 0.0f, FC(0.057f), 1.0f),
                           ab<P>(V0, FC(0.0013f), FC(-0.06f), FC(20.f), 0.0f, 0.0f, FC(-0.04f), 1.0f), inf, tau);
                XI1 = rush_larsen<P>(XI, inf, tau, mdtn);
                inf_tau<P>(ab<P>(V0, FC(0.055f), FC(-.25f), FC(78.0f), 0.0f, 0.0f, FC(-0.2f), 1.0f),
                           ab<P>(V0, FC(0.3f), FC(0.0f), FC(32.f), 0.0f, 0.0f, FC(-0.1f), 1.0f), inf, tau);
                J1 = rush_larsen<P>(J, inf, tau, mdtn);
                inf_tau<P>(ab<P>(V0, FC(2 * 0.095), FC(-0.01f), FC(-5.f), 0.0f, 0.0f, FC(-0.072f), 1.0f),
                           ab<P>(V0, FC(2 * 0.07), FC(-0.017f), FC(44.f), 0.0f, 0.0f, FC(0.05f), 1.0f), inf, tau);
                D1 = rush_larsen<P>(D, inf, tau, mdtn);
                inf_tau<P>(ab<P>(V0, FC(2 * 0.012), FC(-0.008f), FC(28.f), 0.0f, 0.0f, FC(0.15f), 1.0f),
                           ab<P>(V0, FC(2 * 0.0065), FC(-0.02f), FC(30.f), 0.0f, 0.0f, FC(-0.2f), 1.0f), inf, tau);
                F1 = rush_larsen<P>(F, inf, tau, mdtn);
            }
        }
        // currents from the OLD gates, br.py:150-165
        // i_K1's second quotient (V+23) / (1 - exp(-0.04 (V+23))) is 0/0 at V0 == -23.0f and at no other float32 potential;
        // there it is DEFINED as its limit 1/0.04 = 25 under both policies and both gate forms (DESIGN.md 9, "op contract":
        // the reference's NaN ends as V = -85 through the clip) — a select on the finished quotient
        const auto at23 = vcmp_eq(V0, -23.0f);
        if constexpr (same_type<P, Fast>::value) {
            // Fast: the five exponentials of iK1 and ix1 are all powers of ONE e = exp(0.04 V0) times constants
            // (exp(0.08 (V0+53)) = (e*E53)^2, exp(-0.04 (V0+23)) = 1 / (e*E23), ...): one v_exp and three v_rcp instead
            // of five and three — the kernels are issue-bound and a transcendental costs four plain instructions
            constexpr float E85 = FC(29.96410004739701), E53 = FC(8.3311374876876929), E23 = FC(2.5092903899362979),
                            E77 = FC(21.7584023961970), E35 = FC(4.0551999668446745);
            const T e = vmap(V0 * FC(0.04 * 1.44269504088896340736), [](float y) { return __builtin_amdgcn_exp2f(y); });
            const T re = P::rcp(e);
            const T a = e * E53;
            const T t1 = vfma(e, 4.0f * E85, -4.0f) * P::rcp(vfma(a, a, a));          // 4 (e^{.04(V+85)} - 1) / (a^2 + a)
            // (V+23) / (1 - e^{-.04(V+23)}), at V0 == -23.0f DEFINED as its limit 25 (at23 above; the denominator of THIS form
            // need not be an exact zero there, so the quotient without the select could be 0 or NaN)
            const T t2 = vsel(at23, T_of<T>(25.0f), (V0 + 23.0f) * P::rcp(vfma(re, FC(-1.0 / 2.5092903899362979), 1.0f)));
            const T iK1x = vfma(t2, 0.2f, t1);                         // iK1 / 0.35
            const T ix1 = XI * vfma(re, FC(-0.8 / 4.0551999668446745), FC(0.8 * 21.7584023961970 / 4.0551999668446745));   // 0.8 (e*E77 - 1) / (e*E35)
            (void)E23; (void)E35; (void)E77; (void)E85;
            // ... and the same currents with every a*b+c that the reference leaves as two operations written as ONE multiply-add, and
            // log C as the bare v_log_f32 (C is a concentration of 1e-7 .. 1e-5: never subnormal, the library form's range
            // scaling is dead code) with ln 2 and E_Ca's factor folded into the multiply-add behind it: 11 instructions of 222 per
            // cell fewer.  Rounding-level differences only (br.py:150-170).  The factor 4 of the sodium conductance moved into the
            // driving force (a power of two: exact), the calcium conductance's 0.09 into E_Ca's multiply-add.
            const T gNa = vfma(((M * M) * M) * H, J, T_of<T>(0.00125f));
            const T dNa = vfma(V0, 4.0f, -200.0f);
            const T l2C = vmap(C, [](float y) { return __builtin_amdgcn_logf(y); });
            const T dCa = vfma(l2C, FC(0.09 * 13.0278 * 0.69314718055994530942), vfma(V0, FC(0.09), FC(0.09 * 82.3)));   // 0.09 (V - E_Ca)
            const T iCa = (D * F) * dCa;
            const T I_sum = vfma(gNa, dNa, vfma(iK1x, 0.35f, ix1)) + iCa;
            const T V1 = clipf(P::mad(I_sum, -k.dt, P::mad(lap, k.ddt, V0)), -85.0f, 25.0f);   // :167-168
            s[0] = V1;
            s[1] = P::mad(vfma(iCa, -1.0e-7f, vfma(C, -0.07f, FC(0.07 * 1.0e-7))), k.dt, C);      // :170
        } else {
            const T iK1 = 0.35f * (P::div(4.0f * (P::exp(0.04f * (V0 + 85.0f)) - 1.0f),
                                          P::exp(0.08f * (V0 + 53.0f)) + P::exp(0.04f * (V0 + 53.0f))) +
                                   0.2f * vsel(at23, T_of<T>(25.0f), P::div(V0 + 23.0f, 1.0f - P::exp(-0.04f * (V0 + 23.0f)))));
            const T ix1 = P::div((XI * 0.8f) * (P::exp(0.04f * (V0 + 77.0f)) - 1.0f), P::exp(0.04f * (V0 + 35.0f)));
            const T iNa = (1.0f * (((((4.0f * M) * M) * M) * H) * J + 0.005f)) * (V0 - 50.0f);
            const T ECa = FC(0.0 - 82.3) - 13.0278f * P::log(C);
            const T iCa = ((FC(1.0 * 0.09) * D) * F) * (V0 - ECa);
            const T I_sum = ((iK1 + ix1) + iNa) + iCa;
            const T V1 = clipf(P::mad(I_sum, -k.dt, P::mad(lap, k.ddt, V0)), -85.0f, 25.0f);   // :167-168
            const T dC = -1.0e-7f * iCa + 0.07f * (1.0e-7f - C);                                   // :170
            s[0] = V1;
            s[1] = P::mad(dC, k.dt, C);
        }
        s[2] = M1; s[3] = H1; s[4] = J1; s[5] = D1; s[6] = F1; s[7] = XI1;
    
