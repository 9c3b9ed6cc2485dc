// body of Fenton::pre — Fenton's update (fenton.py:46-108) except the potential's own line (Fenton::post).  T is float (one cell) or vf<R> (the R cells a lane
// owns, operation-major): the same arithmetic per cell either way.  P::mad(a,b,c) is (a*b)+c with two
// roundings under Exact and one fused multiply-add under Fast.
        // constants fenton.py:49-71; the divisors appear literally below: tau_d 0.065, tau_si = tau_so
        // 31.8364, c_so 0.02, tau_vp 3.33, tau_vn 19.2, tau_wp 160, tau_wn1 = tau_wn2 75
        constexpr float tau_a = FC(0.009), u_c = FC(0.23), u_w = FC(0.146), u_0 = FC(0.0), u_m = FC(1.0),
                        u_csi = FC(0.8), u_so = FC(0.3), r_sn = FC(1.2), k_ = FC(3.0), b_so = FC(0.84);
        constexpr float half_aso = FC(0.5 * (0.115 - 0.009));   // 0.5*(a_so - tau_a) in double
        constexpr float rsp_m_rsn = FC(0.02 - 1.2);             // (r_sp - r_sn) in double
        if constexpr (same_type<P, Fast>::value) {
            // ---- Fast: the same model with constants folded and every a*b+c one FMA — 35 VALU instructions per
            // cell instead of 49 (the kernels are instruction-issue bound, DESIGN.md 6).  Differences from the
            // rounding-faithful form are reassociations only: within the fast tolerance of the parity tests.
            constexpr float L2E2 = FC(2.0 * 1.44269504088896340736);         // 2*log2(e): tanh through 2^x
            const T U = s[0], V = s[1], W = s[2], S = s[3];                  // raw U: fenton.py:101
            const T a = U - u_c;
            const T Huc = heav(a);                                           // :73-75
            const T b = U - u_so;
            const T Huso = heav(b);                                          // :77-79 (G = 1 - H exactly: the values are 0, 0.5, 1)
            // I_fi = -V*H*(U-u_c)*(u_m-U)/tau_d = (V*H/tau_d) * (a*U - a)     (u_m = 1)                        :81
            const T t1 = (V * Huc) * FC(1.0 / 0.065);
            const T t2 = vfma(a, U, -a);
            // 1 + tanh((U-b_so)/c_so) = 2 - 2*q1,  q1 = 1/(2^(A*U - A*b_so) + 1)                               :83
            const T q1 = P::sigm_q2(vfma(U, FC(2.0 * 1.44269504088896340736 / 0.02), FC(-2.0 * 1.44269504088896340736 / 0.02 * 0.84)));
            T iso = vfma(q1, FC(-2.0 * 0.5 * (0.115 - 0.009)), FC(2.0 * 0.5 * (0.115 - 0.009)));
            // U*G = U - U*H in ONE multiply-add, exact (H is 0, 0.5 or 1): the second Heaviside — a form with a scalar operand, twice
            // the issue cost of a plain one — and its product are gone; bit-identical
            iso = vfma(vfma(-U, Huso, U), FC(1.0 / 31.8364), iso);           // (U - u_0) = U                  :84
            iso = vfma(Huso, tau_a, iso);
            // dU = -(I_fi + I_si + I_so),  I_si = -W*S/tau_si                                                 :82,:86
            const T dU = vfma(-t1, t2, vfma(W * S, FC(1.0 / 31.8364), -iso));
            const auto exc = vgt(U, u_c);
            const T r_s = vfma(Huc, rsp_m_rsn, r_sn);                                                        // :89
            // 0.5*(1 + tanh(k(U-u_csi))) = 1 - q2                                                            :90
            // ... = 1/(1 + 2^-x): the sigmoid itself instead of one minus its complement (one subtraction fewer, and no cancellation
            // where the complement is close to one)
            const T p2 = P::sigm_q2(vfma(U, FC(-2.0 * 1.44269504088896340736 * 3.0), FC(2.0 * 1.44269504088896340736 * 3.0 * 0.8)));
            const T dS = r_s * (p2 - S);
            dU_out = dU;                                                     // the potential's update: Fenton::post
            s[1] = vsel(exc, V * k.cvp, vfma(V, k.cvn, k.dvn));                                              // :87,:105
            s[2] = vsel(exc, W * k.cwp, vfma(W, k.cwn, k.dwn));              // tau_wn1 == tau_wn2           :88,:106
            s[3] = vfma(dS, k.dt, S);
            (void)L2E2; (void)u_w; (void)u_0; (void)u_m; (void)u_csi; (void)k_; (void)b_so; (void)half_aso;
        } else {
        const T U = s[0], V = s[1], W = s[2], S = s[3];         // raw U: fenton.py:101

        const T Huc = heav(U - u_c);                            // H(), :73-75
        const T Huso = heav(U - u_so);                          // G() = 1 - H, :77-79: formed below

        const T I_fi = DC((((-V) * Huc) * (U - u_c)) * (u_m - U), 0.065);                       // :81
        const T I_si = DC((-W) * S, 31.8364);                                                    // :82
        // (H * c is EXACT for H in {0, 0.5, 1}, so the reference's two roundings of H*c + x are the one rounding of a fused
        // multiply-add — same bits, one instruction; likewise (U - u_0) G)
        const T I_so = vfma(Huso, tau_a, P::mad(P::one_plus_tanh(DC(U - b_so, 0.02)), half_aso,
                                                  // (U - u_0) G = U - U H in one multiply-add: exact (u_0 = 0; H is 0, 0.5 or 1), bit-identical
                                                  DC(vfma(-U, Huso, U), 31.8364)));                // :83-84
        const T dU = -((I_fi + I_si) + I_so);                                                    // :86
        const auto exc = vgt(U, u_c);
        const T dV = vsel(exc, DC(-V, 3.33), DC(1.0f - V, 19.2));                                // :87
        const T dW = vsel(exc, DC(-W, 160.0), vsel(vgt(U, u_w), DC(1.0f - W, 75.0), DC(1.0f - W, 75.0)));  // :88
        const T r_s = vfma(Huc, rsp_m_rsn, T_of<T>(r_sn));                                      // :89
        const T dS = r_s * P::half_one_plus_tanh_minus((U - u_csi) * k_, S);                     // :90

        dU_out = dU;                                                                             // :103 -> Fenton::post
        s[1] = P::mad(dV, k.dt, V);
        s[2] = P::mad(dW, k.dt, W);
        s[3] = P::mad(dS, k.dt, S);
        }
