// bfgs_advance.inc -- the body of the protothread of bfgs_machine.h, which includes
// it once per way of obtaining f and the gradient: with BF_SF_FUN / BF_SF_GRAD /
// BF_SF_FUN_GRAD standing for ScalarFunction over forward differences (advance), and
// over a function that returns (f, grad f) from one call (advance_jac).  The
// statements of _minimize_bfgs and its line searches are stated here, once.
// Runs `c` to its next request (c.nrows > 0, c.rows) or to its end (c.done).
// Before every call but the first the caller has written c.vals[0 .. nrows).
BF_HD inline void BF_ADVANCE(Run &c) {
  const int n = c.n;
  c.nrows = 0;
  switch (c.pc) {
    case 0:;
      BF_SF_FUN_GRAD(c.xk);
      c.old_fval = c.f;
      for (int i = 0; i < n; i++) c.gfk[i] = c.g[i];
      c.k = 0, c.warnflag = 0;
      // np.linalg.norm: sqrt of the sum of squares
      c.old_old_fval = c.old_fval + std::sqrt(dot(c.gfk, c.gfk, n)) / 2;
      c.have_old_old = true;
      c.gnorm = 0;
      for (int i = 0; i < n; i++) {
        const double a = std::fabs(c.gfk[i]);
        if (a > c.gnorm || a != a) c.gnorm = a;  // np.amax propagates nan
      }
      while (c.gnorm > c.gtol && c.k < c.maxiter) {
        for (int i = 0; i < n; i++) c.pk[i] = -dot(c.Hk + i * n, c.gfk, n);
        c.alpha_k = 0, c.fval = 0, c.ofv = 0;
        c.have_stp = false, c.have_gnew = false;
        // ---------------- line_search_wolfe1 (amin=1e-100, amax=1e100) ----------
        c.derphi0 = dot(c.gfk, c.pk, n);
        c.phi0 = c.old_fval;
        if (c.have_old_old && c.derphi0 != 0) {
          c.alpha1 = 1.01 * 2 * (c.phi0 - c.old_old_fval) / c.derphi0;
          c.alpha1 = (c.alpha1 < 1.0) ? c.alpha1 : 1.0;  // min(1.0, alpha1)
          if (c.alpha1 < 0) c.alpha1 = 1.0;
        } else {
          c.alpha1 = 1.0;
        }
        c.ds.reset(c.c1, c.c2, 1e-14, 1e-100, 1e100);
        c.phi1 = c.phi0, c.derphi1 = c.derphi0, c.stp = c.alpha1;
        for (int i = 0; i < n; i++) c.gfkp1[i] = c.gfk[i];
        c.task = T_FG;
        c.stp_ok = false;
        for (c.it = 0; c.it < 100; c.it++) {
          c.stp = c.alpha1;
          c.task = c.ds.step(c.stp, c.phi1, c.derphi1);
          if (!std::isfinite(c.stp)) {
            c.task = T_WARN;
            c.stp_ok = false;
            break;
          }
          c.stp_ok = true;
          if (c.task == T_FG) {
            c.alpha1 = c.stp;
            for (int i = 0; i < n; i++) c.xt[i] = c.xk[i] + c.stp * c.pk[i];
            BF_SF_FUN_GRAD(c.xt);
            c.phi1 = c.f;
            for (int i = 0; i < n; i++) c.gfkp1[i] = c.g[i];
            c.derphi1 = dot(c.gfkp1, c.pk, n);
          } else {
            break;
          }
        }
        if (c.it == 100) {
          c.stp_ok = false;
          c.task = T_WARN;
        }
        if (c.task == T_ERROR || c.task == T_WARN) c.stp_ok = false;
        if (c.stp_ok) {
          c.have_stp = true;
          c.alpha_k = c.stp;
          c.fval = c.phi1;
          c.ofv = c.phi0;
          c.have_gnew = true;
        }
        // ---------------- line_search_wolfe2 fall-back ---------------------------
        if (!c.have_stp) {
          c.derphi0 = dot(c.gfk, c.pk, n);
          c.phi0 = c.old_fval;
          c.old_phi0 = c.old_old_fval;
          c.alpha0 = 0;
          if (c.have_old_old && c.derphi0 != 0) {
            c.alpha1 = 1.01 * 2 * (c.phi0 - c.old_phi0) / c.derphi0;
            c.alpha1 = (c.alpha1 < 1.0) ? c.alpha1 : 1.0;
          } else {
            c.alpha1 = 1.0;
          }
          if (c.alpha1 < 0) c.alpha1 = 1.0;
          c.alpha1 = (1e100 < c.alpha1) ? 1e100 : c.alpha1;  // amax
          for (int i = 0; i < n; i++) c.xt[i] = c.xk[i] + c.alpha1 * c.pk[i];
          BF_SF_FUN(c.xt);
          c.phi_a1 = c.f;
          c.phi_a0 = c.phi0, c.derphi_a0 = c.derphi0;
          c.star_alpha = false, c.star_der = false;
          c.alpha_star = 0, c.phi_star = 0;
          c.do_zoom = false;
          c.z_lo = 0, c.z_hi = 0, c.zphi_lo = 0, c.zphi_hi = 0, c.zder_lo = 0;
          c.fell_through = true;
          for (c.i2 = 0; c.i2 < 10; c.i2++) {
            if (c.alpha1 == 0 || c.alpha0 > 1e100) {
              c.star_alpha = false;
              c.phi_star = c.phi0;
              c.star_der = false;
              c.phi0 = c.old_phi0;
              c.fell_through = false;
              break;
            }
            if ((c.phi_a1 > c.phi0 + c.c1 * c.alpha1 * c.derphi0) ||
                ((c.phi_a1 >= c.phi_a0) && c.i2 > 0)) {
              c.do_zoom = true;
              c.z_lo = c.alpha0, c.z_hi = c.alpha1, c.zphi_lo = c.phi_a0,
              c.zphi_hi = c.phi_a1, c.zder_lo = c.derphi_a0;
              c.fell_through = false;
              break;
            }
            for (int q = 0; q < n; q++) c.xt[q] = c.xk[q] + c.alpha1 * c.pk[q];
            BF_SF_GRAD(c.xt);
            for (int q = 0; q < n; q++) c.gfkp1[q] = c.g[q];
            c.derphi_a1 = dot(c.gfkp1, c.pk, n);
            if (std::fabs(c.derphi_a1) <= -c.c2 * c.derphi0) {
              c.star_alpha = true;
              c.alpha_star = c.alpha1;
              c.phi_star = c.phi_a1;
              c.star_der = true;
              c.fell_through = false;
              break;
            }
            if (c.derphi_a1 >= 0) {
              c.do_zoom = true;
              c.z_lo = c.alpha1, c.z_hi = c.alpha0, c.zphi_lo = c.phi_a1,
              c.zphi_hi = c.phi_a0, c.zder_lo = c.derphi_a1;
              c.fell_through = false;
              break;
            }
            {
              double alpha2 = 2 * c.alpha1;
              alpha2 = (1e100 < alpha2) ? 1e100 : alpha2;
              c.alpha0 = c.alpha1;
              c.alpha1 = alpha2;
            }
            c.phi_a0 = c.phi_a1;
            for (int q = 0; q < n; q++) c.xt[q] = c.xk[q] + c.alpha1 * c.pk[q];
            BF_SF_FUN(c.xt);
            c.phi_a1 = c.f;
            c.derphi_a0 = c.derphi_a1;
          }
          if (c.fell_through) {  // the for-else of scalar_search_wolfe2
            c.star_alpha = true;
            c.alpha_star = c.alpha1;
            c.phi_star = c.phi_a1;
            c.star_der = false;
          }
          if (c.do_zoom) {
            c.a_lo = c.z_lo, c.a_hi = c.z_hi, c.phi_lo = c.zphi_lo,
            c.phi_hi = c.zphi_hi, c.derphi_lo = c.zder_lo;
            c.iz = 0;
            c.phi_rec = c.phi0, c.a_rec = 0;
            c.star_alpha = false;
            c.star_der = false;
            while (true) {
              {
                const double delta1 = 0.2, delta2 = 0.1;
                const double dalpha = c.a_hi - c.a_lo;
                double a, b;
                if (dalpha < 0)
                  a = c.a_hi, b = c.a_lo;
                else
                  a = c.a_lo, b = c.a_hi;
                double a_j = 0, cchk = 0;
                bool have_aj = false;
                if (c.iz > 0) {
                  cchk = delta1 * dalpha;
                  have_aj = cubicmin(c.a_lo, c.phi_lo, c.derphi_lo, c.a_hi, c.phi_hi,
                                     c.a_rec, c.phi_rec, a_j);
                }
                if (c.iz == 0 || !have_aj || a_j > b - cchk || a_j < a + cchk) {
                  const double qchk = delta2 * dalpha;
                  have_aj =
                      quadmin(c.a_lo, c.phi_lo, c.derphi_lo, c.a_hi, c.phi_hi, a_j);
                  if (!have_aj || a_j > b - qchk || a_j < a + qchk)
                    a_j = c.a_lo + 0.5 * dalpha;
                }
                c.a_j = a_j;
              }
              for (int q = 0; q < n; q++) c.xt[q] = c.xk[q] + c.a_j * c.pk[q];
              BF_SF_FUN(c.xt);
              c.phi_aj = c.f;
              if ((c.phi_aj > c.phi0 + c.c1 * c.a_j * c.derphi0) ||
                  (c.phi_aj >= c.phi_lo)) {
                c.phi_rec = c.phi_hi, c.a_rec = c.a_hi;
                c.a_hi = c.a_j, c.phi_hi = c.phi_aj;
              } else {
                for (int q = 0; q < n; q++) c.xt[q] = c.xk[q] + c.a_j * c.pk[q];
                BF_SF_GRAD(c.xt);
                for (int q = 0; q < n; q++) c.gfkp1[q] = c.g[q];
                {
                  const double derphi_aj = dot(c.gfkp1, c.pk, n);
                  if (std::fabs(derphi_aj) <= -c.c2 * c.derphi0) {
                    c.star_alpha = true;
                    c.alpha_star = c.a_j;
                    c.phi_star = c.phi_aj;
                    c.star_der = true;
                    break;
                  }
                  if (derphi_aj * (c.a_hi - c.a_lo) >= 0) {
                    c.phi_rec = c.phi_hi, c.a_rec = c.a_hi;
                    c.a_hi = c.a_lo, c.phi_hi = c.phi_lo;
                  } else {
                    c.phi_rec = c.phi_lo, c.a_rec = c.a_lo;
                  }
                  c.a_lo = c.a_j, c.phi_lo = c.phi_aj, c.derphi_lo = derphi_aj;
                }
              }
              c.iz += 1;
              if (c.iz > 10) break;  // (None, None, None)
            }
          }
          if (c.star_alpha) {
            c.have_stp = true;
            c.alpha_k = c.alpha_star;
            c.fval = c.phi_star;
            c.ofv = c.phi0;
            c.have_gnew = c.star_der;  // gval[0] of the last derphi call
          }
        }
        if (!c.have_stp) {
          c.warnflag = 2;
          break;
        }
        c.old_fval = c.fval;
        c.old_old_fval = c.ofv;
        c.have_old_old = true;
        for (int i = 0; i < n; i++) {
          c.sk[i] = c.alpha_k * c.pk[i];
          c.xk[i] = c.xk[i] + c.sk[i];
        }
        if (!c.have_gnew) {
          BF_SF_GRAD(c.xk);
          for (int i = 0; i < n; i++) c.gfkp1[i] = c.g[i];
        }
        for (int i = 0; i < n; i++) {
          c.yk[i] = c.gfkp1[i] - c.gfk[i];
          c.gfk[i] = c.gfkp1[i];
        }
        c.k += 1;
        c.gnorm = 0;
        for (int i = 0; i < n; i++) {
          const double a = std::fabs(c.gfk[i]);
          if (a > c.gnorm || a != a) c.gnorm = a;
        }
        if (c.gnorm <= c.gtol) break;
        {
          double pp = 0, xx = 0;
          for (int i = 0; i < n; i++) pp += c.pk[i] * c.pk[i];
          for (int i = 0; i < n; i++) xx += c.xk[i] * c.xk[i];
          if (c.alpha_k * std::sqrt(pp) <= c.xrtol * (c.xrtol + std::sqrt(xx)))
            break;
        }
        if (!std::isfinite(c.old_fval)) {
          c.warnflag = 2;
          break;
        }
        {
          const double rhok_inv = dot(c.yk, c.sk, n);
          const double rhok = (rhok_inv == 0.) ? 1000.0 : 1. / rhok_inv;
          // Hk = A1 Hk A2 + rhok sk sk^T, A1 = I - sk yk^T rhok, A2 = I - yk sk^T rhok
          // (the entries of A1 / A2 formed where they are used: the same products)
          for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
              double s = 0;
              for (int q = 0; q < n; q++)
                s += c.Hk[i * n + q] *
                     ((q == j ? 1.0 : 0.0) - c.yk[q] * c.sk[j] * rhok);
              c.T1[i * n + j] = s;
            }
          for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
              double s = 0;
              for (int q = 0; q < n; q++)
                s += ((i == q ? 1.0 : 0.0) - c.sk[i] * c.yk[q] * rhok) *
                     c.T1[q * n + j];
              c.Hk[i * n + j] = s + (rhok * c.sk[i]) * c.sk[j];
            }
        }
      }
      c.fval = c.old_fval;
      if (c.warnflag == 2) {
      } else if (c.k >= c.maxiter) {
        c.warnflag = 1;
      } else {
        bool xnan = false;
        for (int i = 0; i < n; i++)
          if (c.xk[i] != c.xk[i]) xnan = true;
        if (c.gnorm != c.gnorm || c.fval != c.fval || xnan) c.warnflag = 3;
      }
      c.nit = c.k;
      c.status = c.warnflag;
      c.nrows = 0;
      c.done = true;
      c.pc = -1;
      return;
    default:
      return;  // finished runs stay finished
  }
}
