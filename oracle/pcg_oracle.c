/*
 * pcg_oracle.c -- CPU restatement of pc-gym's per-timestep hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ is part of the product: only
 * tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load it,
 * and only as the checker / the timed CPU baseline.  The product
 * (pc-gym_amd/, libpcgym_hip.so) never links, imports or falls back to it.
 *
 * Pinning: the reference is pure Python whose integrator arithmetic lives in
 * un-vendored third-party wheels (casadi -> SUNDIALS CVODES, requirements.txt:7;
 * diffrax Tsit5, requirements.txt:8-10), none installed here.  The oracle is
 * therefore pinned by
 *   (1) RHS vectors produced by importing the reference's own model_classes.py
 *       (tests/golden/rhs_*.npz, generator tests/golden/gen_golden.py),
 *   (2) the MPC-oracle trajectories the reference ships in pc-gym_paper
 *       (tests/golden/paper_*.npz; authored by its own CVODES simulator), replayed
 *       as (x,u,dt)->x' known answers,
 *   (3) the reference's only in-tree KAT (custom linear model,
 *       tests/environment/test_make_env_custom_model.py:66-86),
 *   (4) full reset()/step() tuples recorded from the reference make_env with the
 *       CVODES call replaced by LSODA(1e-12) on the reference's own RHS
 *       (tests/golden/step_*.npz),
 *   (5) Random123's published Philox4x32-10 known answers.
 * See tests/test_oracle_golden.py.
 *
 * Each function cites the reference lines it follows.  Arithmetic is written in
 * the reference's own expression order so that RHS values agree to ~1 ulp.
 * The integrators (fixed-step RK4 with sub-steps; adaptive Dormand-Prince 5(4))
 * are NOT the reference's (CVODES BDF / Tsit5): any convergent one-step method
 * reproduces the same ODE solution to the reference's accuracy class
 * (CasADi default reltol 1e-6); see DESIGN.md "Numerical contract".
 *
 * Build: make -C oracle   (gcc -O2 -fopenmp -shared -fPIC) -> oracle/libpcg_oracle.so
 */
#define _GNU_SOURCE /* sched_setaffinity: the timed CPU baseline pins its OpenMP team (orc_pin_threads) */
#include <math.h>
#include <sched.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "../include/pcgym_hip.h"

#define ORC_EXPORT __attribute__((visibility("default")))

/* ------------------------------------------------------------------------- */
/* Model right-hand sides                                                     */
/* ------------------------------------------------------------------------- */

/* model_classes.py:45-62.  p = q,V,rho,C,deltaHr,EA_over_R,k0,UA,Ti,Caf (:24-33).
 * u.size==1 -> Tc only; else Tc,Ti,Caf = u[0..2] (:48-51). */
static void rhs_cstr(const double* p, const double* x, const double* u, int nu, double* dx) {
  double q = p[0], V = p[1], rho = p[2], C = p[3], deltaHr = p[4], EA_over_R = p[5], k0 = p[6],
         UA = p[7], Ti = p[8], Caf = p[9];
  double ca = x[0], T = x[1];
  double Tc = u[0];
  if (nu != 1) {
    Ti = u[1];
    Caf = u[2];
  }
  double rA = k0 * exp(-EA_over_R / T) * ca;
  dx[0] = q / V * (Caf - ca) - rA;
  dx[1] = q / V * (Ti - T) + ((-deltaHr) * rA) * (1 / (rho * C)) + UA * (Tc - T) * (1 / (rho * C * V));
}

/* model_classes.py:891-913.  p = g,gamma_1,gamma_2,k1,k2,a1..a4,A1..A4 (:877-889). */
static void rhs_four_tank(const double* p, const double* x, const double* u, int nu, double* dx) {
  (void)nu;
  double g = p[0], gamma_1 = p[1], gamma_2 = p[2], k1 = p[3], k2 = p[4];
  double a1 = p[5], a2 = p[6], a3 = p[7], a4 = p[8], A1 = p[9], A2 = p[10], A3 = p[11], A4 = p[12];
  double h1 = x[0], h2 = x[1], h3 = x[2], h4 = x[3], v1 = u[0], v2 = u[1];
  dx[0] = (-a1 / A1) * sqrt(2 * g * h1) + (a3 / A1) * sqrt(2 * g * h3) + ((gamma_1 * k1) / (A1)) * v1;
  dx[1] = (-a2 / A2) * sqrt(2 * g * h2) + (a4 / A2) * sqrt(2 * g * h4) + ((gamma_2 * k2) / (A2)) * v2;
  dx[2] = (-a3 / A3) * sqrt(2 * g * h3) + (((1 - gamma_2) * k2) / (A3)) * v2;
  dx[3] = (-a4 / A4) * sqrt(2 * g * h4) + (((1 - gamma_1) * k1) / (A4)) * v1;
}

/* model_classes.py:370-412.  p = Vl,Vg,m,Kla,eq_exponent,X0,Y6 (:361-367).
 * u.size==2 -> L,G; else L,G,X0,Y6 (:382-385).  x = X1,Y1,...,X5,Y5 interleaved. */
static void rhs_me(const double* p, const double* x, const double* u, int nu, double* dx) {
  double Vl = p[0], Vg = p[1], m = p[2], Kla = p[3], e = p[4], X0 = p[5], Y6 = p[6];
  double L = u[0], G = u[1];
  if (nu != 2) {
    X0 = u[2];
    Y6 = u[3];
  }
  double Q[5];
  for (int s = 0; s < 5; ++s) {
    double Xeq = pow(x[2 * s + 1], e) / m;
    Q[s] = Kla * (x[2 * s] - Xeq) * Vl;
  }
  for (int s = 0; s < 5; ++s) {
    double Xprev = (s == 0) ? X0 : x[2 * (s - 1)];
    double Ynext = (s == 4) ? Y6 : x[2 * (s + 1) + 1];
    dx[2 * s] = (1 / Vl) * (L * (Xprev - x[2 * s]) - Q[s]);
    dx[2 * s + 1] = (1 / Vg) * (G * (Ynext - x[2 * s + 1]) + Q[s]);
  }
}

/* The same right-hand side in the KERNEL's operation order (pc-gym_amd/csrc/pcg_models.hpp, MEImpl<true>::rhs:
 * pre-folded constants 1/Vl, 1/Vg, 1/m, Kla Vl; fused multiply-adds where the kernel has them), for eq_exponent == 2.
 * This model runs the adaptive pair at its stability limit, where a last-bit difference of one evaluation changes the
 * step-size sequence a few steps later (tests/helpers.py); with this twin inside the integrator the oracle follows the
 * kernel bit for bit.  It is pinned to rhs_me() -- the reference's own expression order, itself pinned to the
 * reference's vectors -- at 4e-16 relative (tests/test_oracle_golden.py); orc_rhs() keeps reporting rhs_me(). */
static void rhs_me_kernel_order(const double* p, const double* x, const double* u, int nu, double* dx) {
  double iVl = 1 / p[0], iVg = 1 / p[1], inv_m = 1 / p[2], KlaVl = p[3] * p[0], X0 = p[5], Y6 = p[6];
  const double alpha = u[0] * iVl, beta = u[1] * iVg, klap = iVl * KlaVl, eK = iVg * KlaVl; /* folded as the kernel folds them */
  if (nu != 2) {
    X0 = u[2];
    Y6 = u[3];
  }
  for (int s = 0; s < 5; ++s) {
    double X = x[2 * s], Y = x[2 * s + 1];
    double Xp = (s == 0) ? X0 : x[2 * s - 2];
    double Yn = (s == 4) ? Y6 : x[2 * s + 3];
    double q = fma(-(Y * Y), inv_m, X);
    dx[2 * s] = fma(alpha, Xp - X, -(klap * q));
    dx[2 * s + 1] = fma(beta, Yn - Y, eK * q);
  }
}

/* model_classes.py:790-845.  p = Vl,Vg,m,Kla,k,eq_exponent,XA0,YA6,YB6,YC6 (:777-786).
 * x = (XA,YA,YB,YC) x 5 stages. */
static void rhs_me_reactive(const double* p, const double* x, const double* u, int nu, double* dx) {
  (void)nu;
  double Vl = p[0], Vg = p[1], m = p[2], Kla = p[3], k = p[4], e = p[5];
  double XA0 = p[6], YA6 = p[7], YB6 = p[8], YC6 = p[9];
  double L = u[0], G = u[1];
  for (int s = 0; s < 5; ++s) {
    const double* c = x + 4 * s;
    double XA = c[0], YA = c[1], YB = c[2], YC = c[3];
    double XAeq = pow(YA, e) / m;
    double Q = Kla * (XA - XAeq) * Vl;
    double r = k * YA * YB;
    double XAprev = (s == 0) ? XA0 : x[4 * (s - 1)];
    double YAn = (s == 4) ? YA6 : x[4 * (s + 1) + 1];
    double YBn = (s == 4) ? YB6 : x[4 * (s + 1) + 2];
    double YCn = (s == 4) ? YC6 : x[4 * (s + 1) + 3];
    dx[4 * s + 0] = (1 / Vl) * (L * (XAprev - XA) - Q);
    dx[4 * s + 1] = (1 / Vg) * (G * (YAn - YA) + Q - r * Vg);
    dx[4 * s + 2] = (1 / Vg) * (G * (YBn - YB) - r * Vg);
    dx[4 * s + 3] = (1 / Vg) * (G * (YCn - YC) + r * Vg);
  }
}

/* model_classes.py:1295-1319.  p = ka,kb,kc,kd,kg,k1,k2,a,b,alfa,ro (:1260-1270).
 * x = mu0..mu3, conc, CV, Ln ; u = T [degC].  u[1:] ignored (quirk Q13). */
static void rhs_cryst(const double* p, const double* x, const double* u, int nu, double* dx) {
  (void)nu;
  double ka = p[0], kb = p[1], kc = p[2], kd = p[3], kg = p[4], k1 = p[5], k2 = p[6];
  double a = p[7], b = p[8], alfa = p[9], ro = p[10];
  double mu0 = x[0], mu1 = x[1], mu2 = x[2], mu3 = x[3], conc = x[4];
  double T = u[0];
  double Tk = T + 273.15;
  double Ceq = -686.2686 + 3.579165 * Tk - 0.00292874 * (Tk * Tk);
  double S = conc * 1e3 - Ceq;
  double B0 = ka * exp(kb / Tk) * pow(S * S, kc / 2) * pow(mu3 * mu3, kd / 2);
  double Ginf = kg * exp(k1 / Tk) * pow(S * S, k2 / 2);
  double dmi0dt = B0;
  double dmi1dt = Ginf * (a * mu0 + b * mu1 * 1e-4) * 1e4;
  double dmi2dt = 2 * Ginf * (a * mu1 * 1e-4 + b * mu2 * 1e-8) * 1e8;
  double dmi3dt = 3 * Ginf * (a * mu2 * 1e-8 + b * mu3 * 1e-12) * 1e12;
  double dcdt = -0.5 * ro * alfa * Ginf * (a * mu2 * 1e-8 + b * mu3 * 1e-12);
  double CV = sqrt(mu2 * mu0 / (mu1 * mu1) - 1);
  double mu1_2 = mu1 * mu1;
  double dCVdt = 1 / (2 * CV + 1e-10) *
                 ((dmi2dt * mu0 + mu2 * dmi0dt) * mu1_2 - mu2 * mu0 * 2 * mu1 * dmi1dt) /
                 (mu1_2 * mu1_2 + 1e-10);
  double dLndt = (dmi1dt * mu0 - mu1 * dmi0dt) / (mu0 * mu0 + 1e-10);
  dx[0] = dmi0dt;
  dx[1] = dmi1dt;
  dx[2] = dmi2dt;
  dx[3] = dmi3dt;
  dx[4] = dcdt;
  dx[5] = dCVdt;
  dx[6] = dLndt;
}

/* custom_model with an affine RHS (pcgym.py:150-153): dx = A x + B u + c.
 * p = A[nx][nx] | B[nx][nu] | c[nx]. */
static void rhs_affine(const double* p, int nx, const double* x, const double* u, int nu, double* dx) {
  const double* A = p;
  const double* Bm = p + nx * nx;
  const double* c = Bm + nx * nu;
  for (int i = 0; i < nx; ++i) {
    double s = c[i];
    for (int j = 0; j < nx; ++j) s += A[i * nx + j] * x[j];
    for (int j = 0; j < nu; ++j) s += Bm[i * nu + j] * u[j];
    dx[i] = s;
  }
}


/* ---- "next" row f-2: further registry models ------------------------------------------------ */

/* model_classes.py:98-125.  p = q,V,rho,C,deltaHr1,EA1_over_R,k01,deltaHr2,EA2_over_R,k02,UA,Ti,Caf */
static void rhs_complex_cstr(const double* p, const double* x, const double* u, int nu, double* dx) {
  double q = p[0], V = p[1], rho = p[2], C = p[3], deltaHr1 = p[4], EA1 = p[5], k01 = p[6], deltaHr2 = p[7],
         EA2 = p[8], k02 = p[9], UA = p[10], Ti = p[11], Caf = p[12];
  double ca = x[0], cb = x[1], cc = x[2], T = x[3];
  double Tc = u[0];
  if (nu != 1) { Ti = u[1]; Caf = u[2]; }
  double r1 = k01 * exp(-EA1 / T) * ca;
  double r2 = k02 * exp(-EA2 / T) * cb;
  double heat_gen = (-deltaHr1 * r1) + (-deltaHr2 * r2);
  dx[0] = (q / V) * (Caf - ca) - r1;
  dx[1] = (q / V) * (0 - cb) + 2 * r1 - r2;
  dx[2] = (q / V) * (0 - cc) + r2;
  dx[3] = (q / V) * (Ti - T) + heat_gen / (rho * C) + (UA / (rho * C * V)) * (Tc - T);
}

/* model_classes.py:173-183.  p = beta, gamma */
static void rhs_disease(const double* p, const double* x, const double* u, int nu, double* dx) {
  (void)nu;
  double beta = p[0], gamma = p[1], S = x[0], I = x[1], u_in = u[0];
  dx[0] = -beta * S * I - u_in * S;
  dx[1] = beta * S * I - gamma * I;
  dx[2] = gamma * I + u_in * S;
}

/* model_classes.py:248-265.  p = k01,k02,EA1,EA2,R,dH1,dH2,rho,Cp,UA,V */
static void rhs_batch(const double* p, const double* x, const double* u, int nu, double* dx) {
  (void)nu;
  double k01 = p[0], k02 = p[1], EA1 = p[2], EA2 = p[3], R = p[4], dH1 = p[5], dH2 = p[6], rho = p[7], Cp = p[8],
         UA = p[9], V = p[10];
  double CA = x[0], CB = x[1], T = x[3], Tc = u[0];
  double r1 = k01 * exp(-EA1 / (R * T)) * CA;
  double r2 = k02 * exp(-EA2 / (R * T)) * CB;
  dx[0] = -r1;
  dx[1] = 2 * r1 - r2;
  dx[2] = r2;
  dx[3] = -(dH1 * r1 + dH2 * r2) / (rho * Cp) + UA / (rho * Cp * V) * (Tc - T);
}

/* model_classes.py:473-490.  p = u_m,u_d,Y_NX,k_m,k_d,k_sq,K_Nq,k_iq,k_s,k_i,k_N ; u = I, F_N */
static void rhs_photo(const double* p, const double* x, const double* u, int nu, double* dx) {
  (void)nu;
  double u_m = p[0], u_d = p[1], Y_NX = p[2], k_m = p[3], k_d = p[4], k_sq = p[5], K_Nq = p[6], k_iq = p[7],
         k_s = p[8], k_i = p[9], k_N = p[10];
  double c_x = x[0], c_N = x[1], c_q = x[2], I = u[0], F_N = u[1];
  dx[0] = u_m * I / (I + k_s + (I * I / k_i)) * c_x * c_N / (c_N + k_N) - u_d * c_x;
  dx[1] = -Y_NX * u_m * I / (I + k_s + (I * I / k_i)) * c_x * c_N / (c_N + k_N) + F_N;
  dx[2] = k_m * I / (I + k_sq + (I * I / k_iq)) * c_x - (k_d * c_q) / (c_N + K_Nq);
}

/* model_classes.py:646-665.  p = C_O,T_O,V1,V2,U1A1,U2A2,rho,cp,k,E,deltaH,R ; u = F,L,Tc1,Tc2 */
static void rhs_cstr_series(const double* p, const double* x, const double* u, int nu, double* dx) {
  (void)nu;
  double C_O = p[0], T_O = p[1], V1 = p[2], V2 = p[3], U1A1 = p[4], U2A2 = p[5], rho = p[6], cp = p[7], k = p[8],
         E = p[9], deltaH = p[10], R = p[11];
  double C1 = x[0], T1 = x[1], C2 = x[2], T2 = x[3], F = u[0], L = u[1], Tc1 = u[2], Tc2 = u[3];
  dx[0] = (C_O / V1) * F + (1 / V1) * L * C2 - (1 / V1) * (F + L) * C1 - k * C1 * exp((-E / (R * T1)));
  dx[1] = (T_O / V1) * F + (1 / V1) * L * T2 - ((U1A1) / (V1 * rho * cp)) * (T1 - Tc1) - (1 / V1) * (F + L) * T1 +
          ((k * (-deltaH)) / (rho * cp)) * C1 * exp((-E / (R * T1)));
  dx[2] = (1 / V2) * (F + L) * (C1 - C2) - k * C2 * exp((-E / (R * T2)));
  dx[3] = (1 / V2) * (F + L) * (T1 - T2) - ((U2A2) / (V2 * rho * cp)) * (T2 - Tc2) +
          ((k * (-deltaH)) / (rho * cp)) * C2 * exp((-E / (R * T2)));
}

/* model_classes.py:707-745.  p = D,q,alpha,X_feed,M0,Mb,M ; x = X0,X1,X2,X3,Xf,X4,X5,X6,Xb ; u = R,F */
static void rhs_distillation(const double* p, const double* x, const double* u, int nu, double* dx) {
  (void)nu;
  double D = p[0], q = p[1], alpha = p[2], X_feed = p[3], M0 = p[4], Mb = p[5], M = p[6];
  double X0 = x[0], X1 = x[1], X2 = x[2], X3 = x[3], Xf = x[4], X4 = x[5], X5 = x[6], X6 = x[7], Xb = x[8];
  double Rr = u[0], F = u[1];
  double L = Rr * D, V = (Rr + 1) * D, L_dash = L + q * F, V_dash = V + (1 - q) * F, W = F - D;
  double Y1 = (alpha * X1) / (1 + (alpha - 1) * X1), Y2 = (alpha * X2) / (1 + (alpha - 1) * X2);
  double Y3 = (alpha * X3) / (1 + (alpha - 1) * X3), Yf = (alpha * Xf) / (1 + (alpha - 1) * Xf);
  double Y4 = (alpha * X4) / (1 + (alpha - 1) * X4), Y5 = (alpha * X5) / (1 + (alpha - 1) * X5);
  double Y6 = (alpha * X6) / (1 + (alpha - 1) * X6), Yb = (alpha * Xb) / (1 + (alpha - 1) * Xb);
  dx[0] = (1 / M0) * ((V * Y1) - (L + D) * X0);
  dx[1] = (1 / M) * (L * (X0 - X1) + V * (Y2 - Y1));
  dx[2] = (1 / M) * (L * (X1 - X2) + V * (Y3 - Y2));
  dx[3] = (1 / M) * (L * (X2 - X3) + V * (Yf - Y3));
  dx[4] = (1 / M) * (L * X3 - L_dash * Xf + V_dash * Y4 - V * Yf + F * X_feed);
  dx[5] = (1 / M) * (L_dash * (Xf - X4) + V_dash * (Y5 - Y4));
  dx[6] = (1 / M) * (L_dash * (X4 - X5) + V_dash * (Y6 - Y5));
  dx[7] = (1 / M) * (L_dash * (X5 - X6) + V_dash * (Yb - Y6));
  dx[8] = (1 / Mb) * (L_dash * X6 - W * Xb - V_dash * Yb);
}

/* model_classes.py:1197-1213.  p = Ap,Ad,At,Ep_over_R,Ed_over_R,Et_over_R,f,V,deltaHp,rho,cp ; x = T,M,I ; u = F,Tf,Mf,If */
static void rhs_polymer(const double* p, const double* x, const double* u, int nu, double* dx) {
  (void)nu;
  double Ap = p[0], Ad = p[1], At = p[2], Ep = p[3], Ed = p[4], Et = p[5], f = p[6], V = p[7], deltaHp = p[8],
         rho = p[9], cp = p[10];
  double T = x[0], M = x[1], I = x[2], F = u[0], Tf = u[1], Mf = u[2], If = u[3];
  double kp = Ap * exp(-Ep / T), kd = Ad * exp(-Ed / T), kt = At * exp(-Et / T);
  double ri = 2 * f * kd * I;
  double rp = kp * pow((f * kd * I) / kt, 0.5);
  dx[0] = (F / V) * (Tf - T) + ((-deltaHp) / (rho * cp)) * rp;
  dx[1] = (F / V) * (Mf - M) - rp;
  dx[2] = (F / V) * (If - I) - ri;
}

/* model_classes.py:1076-1139.  p = V,Va,Kla,m,eq_exponent,O_air,vm_1,vm_2,K1,K2,KO_1,KO_2 ;
 * x = S1_1,S2_1,S3_1,O_1, ..._2, ..._3, S1_A,S2_A,S3_A,O_A ; u = F,Fr,S1_F,S2_F,S3_F */
static void rhs_biofilm(const double* p, const double* x, const double* u, int nu, double* dx) {
  (void)nu;
  double V = p[0], Va = p[1], Kla = p[2], m = p[3], eq_exponent = p[4], O_air = p[5], vm_1 = p[6], vm_2 = p[7],
         K1 = p[8], K2 = p[9], KO_1 = p[10], KO_2 = p[11];
  double F = u[0], Fr = u[1], S1_F = u[2], S2_F = u[3], S3_F = u[4];
  const double *A = x + 12;
  for (int s = 0; s < 3; ++s) {
    const double *c = x + 4 * s, *up = (s == 0) ? A : x + 4 * (s - 1);
    double S1 = c[0], S2 = c[1], S3 = c[2], O = c[3];
    double r1 = ((vm_1 * S1) / (K1 + S1)) * ((O) / (KO_1 + O));
    double r2 = ((vm_2 * S2) / (K2 + S2)) * ((O) / (KO_2 + O));
    double ro = -r1 * 3.5 - r2 * 1.1;
    double rs1 = -r1, rs2 = +r1 - r2, rs3 = r2;
    dx[4 * s + 0] = (Fr / V) * (up[0] - S1) - rs1;
    dx[4 * s + 1] = (Fr / V) * (up[1] - S2) - rs2;
    dx[4 * s + 2] = (Fr / V) * (up[2] - S3) - rs3;
    dx[4 * s + 3] = (Fr / V) * (up[3] - O) - ro;
  }
  double O_Aeq = (pow(O_air, eq_exponent) / m);
  dx[12] = (Fr / Va) * (x[8] - A[0]) + (F / Va) * (S1_F - A[0]);
  dx[13] = (Fr / Va) * (x[9] - A[1]) + (F / Va) * (S2_F - A[1]);
  dx[14] = (Fr / Va) * (x[10] - A[2]) + (F / Va) * (S3_F - A[2]);
  dx[15] = (Fr / Va) * (x[11] - A[3]) + Kla * (O_Aeq - A[3]);
}

/* model_classes.py:963-1029.  p = Utm,Usm,L,Dt,Dm,Ds,cpt,cpm,cps,rhot,rhom,rhos ;
 * x = Tt1,Tm1,Ts1,...,Tt8,Tm8,Ts8 ; u = Ft,Fs,Tt0,Ts9 */
static void rhs_heat_exchanger(const double* p, const double* x, const double* u, int nu, double* dx) {
  (void)nu;
  double Utm = p[0], Usm = p[1], L = p[2], Dt = p[3], Dm = p[4], Ds = p[5], cpt = p[6], cpm = p[7], cps = p[8],
         rhot = p[9], rhom = p[10], rhos = p[11];
  double Ft = u[0], Fs = u[1], Tt0 = u[2], Ts9 = u[3];
  const double M_PI_ = 3.14159265358979323846; /* numpy.pi */
  double Vt = L * M_PI_ * (Dt * Dt), At = L * M_PI_ * Dt, Vm = L * M_PI_ * (Dm * Dm - Dt * Dt), Am = L * M_PI_ * Dm;
  double Vs = L * M_PI_ * (Ds * Ds - Dm * Dm);
  for (int i = 0; i < 8; ++i) {
    double Tt = x[3 * i], Tm = x[3 * i + 1], Ts = x[3 * i + 2];
    double Qt = Utm * At * (Tt - Tm), Qm = Usm * Am * (Tm - Ts);
    double Tt_in = (i == 0) ? Tt0 : x[3 * (i - 1)];
    double Ts_in = (i == 7) ? Ts9 : x[3 * (i + 1) + 2];
    dx[3 * i] = (1 / (cpt * rhot * Vt)) * (Ft * cpt * (Tt_in - Tt) - Qt);
    dx[3 * i + 1] = (1 / (cpm * rhom * Vm)) * (Qt - Qm);
    dx[3 * i + 2] = (1 / (cps * rhos * Vs)) * (Fs * cps * (Ts_in - Ts) + Qm);
  }
}

/* model_classes.py:283-291.  p = k1f,k1r,k2f,k2r ; x = xA,xB,xC,xD ; the model has no inputs (u ignored) */
static void rhs_invariant_batch(const double* p, const double* x, const double* u, int nu, double* dx) {
  (void)nu; (void)u;
  double k1f = p[0], k1r = p[1], k2f = p[2], k2r = p[3], xA = x[0], xB = x[1], xC = x[2], xD = x[3];
  dx[0] = -(k1f * xA * xB - k1r * xC) - (k2f * xA * xC - k2r * xD);
  dx[1] = -(k1f * xA * xB - k1r * xC);
  dx[2] = (k1f * xA * xB - k1r * xC) - (k2f * xA * xC - k2r * xD);
  dx[3] = k2f * xA * xC - k2r * xD;
}

/* model_classes.py:201-216.  p = N,k,m (N = 10) ; x = positions[10], momenta[10] ; no inputs (u ignored) */
static void rhs_oscillators(const double* p, const double* x, const double* u, int nu, double* dx) {
  (void)nu; (void)u;
  int N = 10;
  double k = p[1], m = p[2];
  for (int i = 0; i < N; ++i) {
    double left = x[(i - 1 + N) % N], right = x[(i + 1) % N];
    dx[i] = x[N + i] / m;
    dx[N + i] = -k * (2 * x[i] - left - right);
  }
}

typedef struct {
  int model_id, nx, nu;
  const double* p;
} orc_model;

/* PCG_MODEL_USER (custom_model with an arbitrary right-hand side, pcgym.py:150-153): the tests compile the SAME C
 * statements the plan hands to hipRTC (pcg_env_cfg.user_rhs_src) with gcc into a small shared object and register the
 * resulting function here -- the oracle has no expression evaluator of its own. */
typedef void (*orc_user_rhs_fn)(const double* x, const double* u, const double* p, double* dx);
static orc_user_rhs_fn g_user_rhs = 0;
ORC_EXPORT void orc_set_user_rhs(orc_user_rhs_fn f) { g_user_rhs = f; }

static void rhs(const orc_model* m, const double* x, const double* u, double* dx) {
  switch (m->model_id) {
    case PCG_MODEL_CSTR: rhs_cstr(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_FOUR_TANK: rhs_four_tank(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_ME: rhs_me(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_ME_REACTIVE: rhs_me_reactive(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_CRYST: rhs_cryst(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_COMPLEX_CSTR: rhs_complex_cstr(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_DISEASE: rhs_disease(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_BATCH: rhs_batch(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_PHOTO: rhs_photo(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_CSTR_SERIES: rhs_cstr_series(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_DISTILLATION: rhs_distillation(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_POLYMER: rhs_polymer(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_BIOFILM: rhs_biofilm(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_HEAT_EX: rhs_heat_exchanger(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_INV_BATCH: rhs_invariant_batch(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_OSCILLATORS: rhs_oscillators(m->p, x, u, m->nu, dx); break;
    case PCG_MODEL_USER:
      if (g_user_rhs) g_user_rhs(x, u, m->p, dx);
      else for (int i = 0; i < m->nx; ++i) dx[i] = NAN; /* not registered: poison, never a silent zero */
      break;
    default: rhs_affine(m->p, m->nx, x, u, m->nu, dx); break;
  }
}

/* the right-hand side as the INTEGRATORS evaluate it: the reference's expression order, except for the extraction
 * model with eq_exponent == 2, which uses the kernel-order twin (see rhs_me_kernel_order) unless switched off */
static int g_me_kernel_order = 1;
ORC_EXPORT void orc_set_me_kernel_order(int on) { g_me_kernel_order = on; }
static void rhs_int(const orc_model* m, const double* x, const double* u, double* dx) {
  if (m->model_id == PCG_MODEL_ME && g_me_kernel_order && m->p[4] == 2.0) rhs_me_kernel_order(m->p, x, u, m->nu, dx);
  else rhs(m, x, u, dx);
}
ORC_EXPORT void orc_rhs_me_kernel_order(const double* p, const double* x, const double* u, int nu, double* dx) {
  rhs_me_kernel_order(p, x, u, nu, dx);
}

/* ------------------------------------------------------------------------- */
/* Integrators over one env step [0,dt], u held constant (integrator.py:163-182:
 * dae = {x, p=u, ode}, t0=0, tf=dt  => zero-order hold)                        */
/* ------------------------------------------------------------------------- */
#define MAXNX PCG_MAX_NX

static void rk4(const orc_model* m, double* x, const double* u, double dt, int nsub) {
  int nx = m->nx;
  double h = dt / nsub;
  double k1[MAXNX], k2[MAXNX], k3[MAXNX], k4[MAXNX], y[MAXNX];
  for (int s = 0; s < nsub; ++s) {
    rhs_int(m, x, u, k1);
    for (int i = 0; i < nx; ++i) y[i] = x[i] + 0.5 * h * k1[i];
    rhs_int(m, y, u, k2);
    for (int i = 0; i < nx; ++i) y[i] = x[i] + 0.5 * h * k2[i];
    rhs_int(m, y, u, k3);
    for (int i = 0; i < nx; ++i) y[i] = x[i] + h * k3[i];
    rhs_int(m, y, u, k4);
    for (int i = 0; i < nx; ++i) x[i] = x[i] + (h / 6.0) * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
  }
}

/* Guard of the fixed-step plan of the cstr (PCG_INT_RK4G; twin of Model<PCG_MODEL_CSTR>::guard): growth rate of the thermal
 * feedback g = d(dT/dt)/dT and a bound rho of the fastest rate, from model_classes.py:45-62's terms. */
static int guard_ok(const orc_model* m, const double* x, double h, double lim, int* calm, int* slow) {
  if (m->model_id != PCG_MODEL_CSTR) { *calm = 0; return 0; }
  const double* p = m->p;
  double q = p[0], V = p[1], rho_ = p[2], C = p[3], deltaHr = p[4], EA_over_R = p[5], k0 = p[6], UA = p[7];
  double ca = x[0], T = x[1];
  double z = (-EA_over_R) / T; /* EA/T^2 = z^2 / EA: no second division (the device computes z for the Arrhenius factor) */
  double kk = k0 * exp(z);
  double fb = ((((-deltaHr) * (1 / (rho_ * C))) * (kk * ca)) * (z * z)) * (1.0 / EA_over_R);
  double base = q / V + UA * (1 / (rho_ * C * V));
  double g = fb - base, rr = kk + fb + base;
  if (!(g <= 0.0)) *calm = 0;                      /* growth, or NaN */
  if (!(rr * h <= lim || !(rr == rr))) *slow = 0;  /* unresolved fastest rate */
  return 1;
}
static int dopri5(const orc_model* m, double* x, const double* u, double dt, double rtol, double atol, int max_steps,
                  int32_t* nacc, int32_t* nrej);
/* guarded RK4: rk4() while the guard holds at every sub-step start and at the end state; otherwise the adaptive pair from
 * the start state at the plan's tolerance (round 3: 1e-7 when only the fastest rate is unresolved
 * (contracting stiff state: local errors do not grow).  Twin of the PCG_INT_RK4G branch of integrate_env in pcg_kernels.hpp */
static int rk4g(const orc_model* m, double* x, const double* u, double dt, int nsub, double rtol, double atol, int max_steps,
                int32_t* nacc, int32_t* nrej) {
  int nx = m->nx;
  double h = dt / nsub;
  double x0[PCG_MAX_NX], k1[PCG_MAX_NX], k2[PCG_MAX_NX], k3[PCG_MAX_NX], k4[PCG_MAX_NX], y[PCG_MAX_NX];
  int calm = 1, slow = 1;
  for (int i = 0; i < nx; ++i) x0[i] = x[i];
  for (int s = 0; s <= nsub; ++s) {
    guard_ok(m, x, h, 1.0, &calm, &slow);
    if (s == nsub) break;
    rhs_int(m, x, u, k1);
    for (int i = 0; i < nx; ++i) y[i] = x[i] + 0.5 * h * k1[i];
    rhs_int(m, y, u, k2);
    for (int i = 0; i < nx; ++i) y[i] = x[i] + 0.5 * h * k2[i];
    rhs_int(m, y, u, k3);
    for (int i = 0; i < nx; ++i) y[i] = x[i] + h * k3[i];
    rhs_int(m, y, u, k4);
    for (int i = 0; i < nx; ++i) x[i] = x[i] + (h / 6.0) * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
  }
  if (nacc) *nacc = 0;
  if (nrej) *nrej = 0;
  if (calm && slow) return 0;
  for (int i = 0; i < nx; ++i) x[i] = x0[i];
  return dopri5(m, x, u, dt, rtol, atol, max_steps, nacc, nrej);
}

/* Dormand & Prince (1980) 5(4) pair, FSAL.  Controller = the spec in DESIGN.md
 * "adaptive stepping": RMS error norm over scale = atol + rtol*max(|y|,|ynew|),
 * accept iff E < 1, factor = clip(0.9*E^-1/5, 0.2, 10) (<=1 right after a
 * rejection), Hairer's initial-step heuristic.  Mirrors the *semantics* of
 * integrator.py:56-61 (adaptive explicit 5(4) pair, rtol=atol=1e-8, dt0=None). */
static double rms_scaled(const double* v, const double* y0, const double* y1, int n, double rtol, double atol) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) {
    double a0 = fabs(y0[i]), a1 = fabs(y1[i]);
    double sc = atol + rtol * (a0 > a1 ? a0 : a1);
    double r = v[i] / sc;
    s += r * r;
  }
  return sqrt(s / n);
}

/* Stage combinations as explicit fused multiply-adds in a fixed order: the twin of lc1..lc6 / axpy in
 * pc-gym_amd/csrc/pcg_integrators.hpp.  The integrator's arithmetic is an exactly specified sequence of IEEE operations
 * on both sides (this file is compiled with -ffp-contract=off; fma() is correctly rounded with or without hardware
 * support), so that the states -- and with them the step-size sequences -- agree bit for bit. */
static double lc1(double c1, double k1) { return c1 * k1; }
static double lc2(double c1, double k1, double c2, double k2) { return fma(c2, k2, c1 * k1); }
static double lc3(double c1, double k1, double c2, double k2, double c3, double k3) { return fma(c3, k3, lc2(c1, k1, c2, k2)); }
static double lc4(double c1, double k1, double c2, double k2, double c3, double k3, double c4, double k4) {
  return fma(c4, k4, lc3(c1, k1, c2, k2, c3, k3));
}
static double lc5(double c1, double k1, double c2, double k2, double c3, double k3, double c4, double k4, double c5,
                  double k5) {
  return fma(c5, k5, lc4(c1, k1, c2, k2, c3, k3, c4, k4));
}
static double lc6(double c1, double k1, double c2, double k2, double c3, double k3, double c4, double k4, double c5,
                  double k5, double c6, double k6) {
  return fma(c6, k6, lc5(c1, k1, c2, k2, c3, k3, c4, k4, c5, k5));
}
static double axpy(double h, double s, double x) { return fma(h, s, x); }
/* x + c1 k1 + ... + cN kN, left to right from x, the step size folded into the coefficients: twin of xlc1..xlc5 */
static double xlc1(double x, double c1, double k1) { return fma(c1, k1, x); }
static double xlc2(double x, double c1, double k1, double c2, double k2) { return fma(c2, k2, xlc1(x, c1, k1)); }
static double xlc3(double x, double c1, double k1, double c2, double k2, double c3, double k3) { return fma(c3, k3, xlc2(x, c1, k1, c2, k2)); }
static double xlc4(double x, double c1, double k1, double c2, double k2, double c3, double k3, double c4, double k4) {
  return fma(c4, k4, xlc3(x, c1, k1, c2, k2, c3, k3));
}
static double xlc5(double x, double c1, double k1, double c2, double k2, double c3, double k3, double c4, double k4, double c5,
                   double k5) {
  return fma(c5, k5, xlc4(x, c1, k1, c2, k2, c3, k3, c4, k4));
}

/* Step-size factors are quantised to 6 mantissa bits (truncation) -- part of the controller's specification
 * (DESIGN.md "Adaptive stepping"): the grid makes the step-size sequence independent of how E^(-1/5) is evaluated
 * (this double pow() here, the fp32 log2/exp2 units in the kernels), so both sides take bit-identical steps. */
static double qtrunc6(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  b &= ~((UINT64_C(1) << 46) - 1);
  memcpy(&v, &b, 8);
  return v;
}

static int dopri5(const orc_model* m, double* x, const double* u, double dt, double rtol, double atol,
                  int max_steps, int32_t* nacc, int32_t* nrej) {
  static const double c2 = 1.0 / 5, c3 = 3.0 / 10, c4 = 4.0 / 5, c5 = 8.0 / 9;
  static const double a21 = 1.0 / 5;
  static const double a31 = 3.0 / 40, a32 = 9.0 / 40;
  static const double a41 = 44.0 / 45, a42 = -56.0 / 15, a43 = 32.0 / 9;
  static const double a51 = 19372.0 / 6561, a52 = -25360.0 / 2187, a53 = 64448.0 / 6561, a54 = -212.0 / 729;
  static const double a61 = 9017.0 / 3168, a62 = -355.0 / 33, a63 = 46732.0 / 5247, a64 = 49.0 / 176,
                      a65 = -5103.0 / 18656;
  static const double b1 = 35.0 / 384, b3 = 500.0 / 1113, b4 = 125.0 / 192, b5 = -2187.0 / 6784, b6 = 11.0 / 84;
  /* e = b - bhat */
  static const double e1 = 71.0 / 57600, e3 = -71.0 / 16695, e4 = 71.0 / 1920, e5 = -17253.0 / 339200,
                      e6 = 22.0 / 525, e7 = -1.0 / 40;
  (void)c2; (void)c3; (void)c4; (void)c5;
  int nx = m->nx;
  /* the tableau rows with the step size folded into the coefficients where that is cheaper (dp5_fold() in
   * pcg_integrators.hpp: by the kernel's compile-time state count -- 8 for the padded affine model) */
  const int fold = (nx > 4 && nx <= 16) || m->model_id == PCG_MODEL_AFFINE;
  double k1[MAXNX], k2[MAXNX], k3[MAXNX], k4[MAXNX], k5[MAXNX], k6[MAXNX], k7[MAXNX];
  double y[MAXNX], ynew[MAXNX], err[MAXNX];
  int acc = 0, rej = 0;
  rhs_int(m, x, u, k1);
  /* initial step (Hairer, Norsett & Wanner II.4) */
  double h;
  {
    double d0 = rms_scaled(x, x, x, nx, rtol, atol);
    double d1 = rms_scaled(k1, x, x, nx, rtol, atol);
    double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    if (h0 > dt) h0 = dt;
    for (int i = 0; i < nx; ++i) y[i] = axpy(h0, k1[i], x[i]);
    rhs_int(m, y, u, k2);
    for (int i = 0; i < nx; ++i) err[i] = k2[i] - k1[i];
    double d2 = rms_scaled(err, x, x, nx, rtol, atol) / h0;
    double dm = d1 > d2 ? d1 : d2;
    double h1 = (dm <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : qtrunc6(pow(0.01 / dm, 0.2));
    h = qtrunc6(fmin(100.0 * h0, h1));
    if (h > dt) h = dt;
  }
  double t = 0.0;
  int rejected_last = 0;
  int status = 0;
  for (;;) {
    int last = 0;
    if (acc + rej >= max_steps) { status = 1; break; }
    if (t + h >= dt * (1.0 - 1e-14)) { h = dt - t; last = 1; }
    if (fold) { /* x + (h a_i1) k1 + ...: the coefficients times the step size, once per attempt (dp5_row<true>) */
      const double ha21 = h * a21, ha31 = h * a31, ha32 = h * a32, ha41 = h * a41, ha42 = h * a42, ha43 = h * a43;
      const double ha51 = h * a51, ha52 = h * a52, ha53 = h * a53, ha54 = h * a54;
      const double ha61 = h * a61, ha62 = h * a62, ha63 = h * a63, ha64 = h * a64, ha65 = h * a65;
      const double hb1 = h * b1, hb3 = h * b3, hb4 = h * b4, hb5 = h * b5, hb6 = h * b6;
      const double he1 = h * e1, he3 = h * e3, he4 = h * e4, he5 = h * e5, he6 = h * e6, he7 = h * e7;
      for (int i = 0; i < nx; ++i) y[i] = xlc1(x[i], ha21, k1[i]);
      rhs_int(m, y, u, k2);
      for (int i = 0; i < nx; ++i) y[i] = xlc2(x[i], ha31, k1[i], ha32, k2[i]);
      rhs_int(m, y, u, k3);
      for (int i = 0; i < nx; ++i) y[i] = xlc3(x[i], ha41, k1[i], ha42, k2[i], ha43, k3[i]);
      rhs_int(m, y, u, k4);
      for (int i = 0; i < nx; ++i) y[i] = xlc4(x[i], ha51, k1[i], ha52, k2[i], ha53, k3[i], ha54, k4[i]);
      rhs_int(m, y, u, k5);
      for (int i = 0; i < nx; ++i) y[i] = xlc5(x[i], ha61, k1[i], ha62, k2[i], ha63, k3[i], ha64, k4[i], ha65, k5[i]);
      rhs_int(m, y, u, k6);
      for (int i = 0; i < nx; ++i) ynew[i] = xlc5(x[i], hb1, k1[i], hb3, k3[i], hb4, k4[i], hb5, k5[i], hb6, k6[i]);
      rhs_int(m, ynew, u, k7);
      for (int i = 0; i < nx; ++i) err[i] = lc6(he1, k1[i], he3, k3[i], he4, k4[i], he5, k5[i], he6, k6[i], he7, k7[i]);
    } else { /* x + h (a_i1 k1 + ...) (dp5_row<false>) */
      for (int i = 0; i < nx; ++i) y[i] = axpy(h, lc1(a21, k1[i]), x[i]);
      rhs_int(m, y, u, k2);
      for (int i = 0; i < nx; ++i) y[i] = axpy(h, lc2(a31, k1[i], a32, k2[i]), x[i]);
      rhs_int(m, y, u, k3);
      for (int i = 0; i < nx; ++i) y[i] = axpy(h, lc3(a41, k1[i], a42, k2[i], a43, k3[i]), x[i]);
      rhs_int(m, y, u, k4);
      for (int i = 0; i < nx; ++i) y[i] = axpy(h, lc4(a51, k1[i], a52, k2[i], a53, k3[i], a54, k4[i]), x[i]);
      rhs_int(m, y, u, k5);
      for (int i = 0; i < nx; ++i) y[i] = axpy(h, lc5(a61, k1[i], a62, k2[i], a63, k3[i], a64, k4[i], a65, k5[i]), x[i]);
      rhs_int(m, y, u, k6);
      for (int i = 0; i < nx; ++i) ynew[i] = axpy(h, lc5(b1, k1[i], b3, k3[i], b4, k4[i], b5, k5[i], b6, k6[i]), x[i]);
      rhs_int(m, ynew, u, k7);
      for (int i = 0; i < nx; ++i) err[i] = h * lc6(e1, k1[i], e3, k3[i], e4, k4[i], e5, k5[i], e6, k6[i], e7, k7[i]);
    }
    double E = rms_scaled(err, x, ynew, nx, rtol, atol);
    if (E < 1.0) {
      double f = (E == 0.0) ? 10.0 : fmin(10.0, fmax(0.2, qtrunc6(0.9 * pow(E, -0.2))));
      if (rejected_last && f > 1.0) f = 1.0;
      t += h;
      h *= f;
      for (int i = 0; i < nx; ++i) { x[i] = ynew[i]; k1[i] = k7[i]; }
      rejected_last = 0;
      ++acc;
      if (last) break; /* reached dt */
    } else {
      /* also the NaN path: E is NaN -> comparison false -> shrink hardest */
      double f = (E == E) ? fmax(0.2, qtrunc6(0.9 * pow(E, -0.2))) : 0.2;
      if (f > 1.0) f = 1.0;
      h *= f;
      rejected_last = 1;
      ++rej;
      if (!(h > 1e-13 * dt)) { status = 2; break; } /* step size underflow (NaN / blow-up) */
    }
  }
  if (nacc) *nacc = acc;
  if (nrej) *nrej = rej;
  if (status != 0) /* gave up at some t < dt: never hand back a partially integrated state (CVODES would raise) */
    for (int i = 0; i < nx; ++i) x[i] = NAN;
  return status;
}

static double lc7(double c1, double k1, double c2, double k2, double c3, double k3, double c4, double k4, double c5,
                  double k5, double c6, double k6, double c7, double k7) {
  return fma(c7, k7, lc6(c1, k1, c2, k2, c3, k3, c4, k4, c5, k5, c6, k6));
}
/* Tsit5 -- Tsitouras (2011) 5(4) pair, FSAL: the method of the reference's jax path (integrator.py:56-61, diffrax.Tsit5
 * under PIDController(rtol = atol = 1e-8)).  Controller, norm, initial step and failure semantics of dopri5() above; twin
 * of tsit5() in pc-gym_amd/csrc/pcg_integrators.hpp, statement by statement.  The coefficients are pinned by their order
 * conditions (tests/test_tsit5.py: 17 rooted trees up to order 5 for b, 8 up to order 4 for the embedded weights). */
static const double T5_A[7][6] = {
    {0},
    {0.161},
    {-0.008480655492356989, 0.335480655492357},
    {2.8971530571054935, -6.359448489975075, 4.3622954328695815},
    {5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525},
    {5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383},
    {0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774}};
static const double T5_E[7] = {-0.00178001105222577714, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629,
                               0.5823571654525552, -0.45808210592918697, 0.015151515151515152};
ORC_EXPORT void orc_tsit5_tableau(double* a42, double* e7) {
  memcpy(a42, T5_A, sizeof T5_A);
  memcpy(e7, T5_E, sizeof T5_E);
}
static int tsit5(const orc_model* m, double* x, const double* u, double dt, double rtol, double atol, int max_steps,
                 int32_t* nacc, int32_t* nrej) {
  int nx = m->nx;
  double k1[MAXNX], k2[MAXNX], k3[MAXNX], k4[MAXNX], k5[MAXNX], k6[MAXNX], k7[MAXNX];
  double y[MAXNX], ynew[MAXNX], err[MAXNX];
  const double(*a)[6] = T5_A;
  const double* e = T5_E;
  int acc = 0, rej = 0;
  rhs_int(m, x, u, k1);
  double h;
  {
    double d0 = rms_scaled(x, x, x, nx, rtol, atol);
    double d1 = rms_scaled(k1, x, x, nx, rtol, atol);
    double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    if (h0 > dt) h0 = dt;
    for (int i = 0; i < nx; ++i) y[i] = axpy(h0, k1[i], x[i]);
    rhs_int(m, y, u, k2);
    for (int i = 0; i < nx; ++i) err[i] = k2[i] - k1[i];
    double d2 = rms_scaled(err, x, x, nx, rtol, atol) / h0;
    double dm = d1 > d2 ? d1 : d2;
    double h1 = (dm <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : qtrunc6(pow(0.01 / dm, 0.2));
    h = qtrunc6(fmin(100.0 * h0, h1));
    if (h > dt) h = dt;
  }
  double t = 0.0;
  int rejected_last = 0, status = 0;
  for (;;) {
    int last = 0;
    if (acc + rej >= max_steps) { status = 1; break; }
    if (t + h >= dt * (1.0 - 1e-14)) { h = dt - t; last = 1; }
    for (int i = 0; i < nx; ++i) y[i] = axpy(h, lc1(a[1][0], k1[i]), x[i]);
    rhs_int(m, y, u, k2);
    for (int i = 0; i < nx; ++i) y[i] = axpy(h, lc2(a[2][0], k1[i], a[2][1], k2[i]), x[i]);
    rhs_int(m, y, u, k3);
    for (int i = 0; i < nx; ++i) y[i] = axpy(h, lc3(a[3][0], k1[i], a[3][1], k2[i], a[3][2], k3[i]), x[i]);
    rhs_int(m, y, u, k4);
    for (int i = 0; i < nx; ++i) y[i] = axpy(h, lc4(a[4][0], k1[i], a[4][1], k2[i], a[4][2], k3[i], a[4][3], k4[i]), x[i]);
    rhs_int(m, y, u, k5);
    for (int i = 0; i < nx; ++i)
      y[i] = axpy(h, lc5(a[5][0], k1[i], a[5][1], k2[i], a[5][2], k3[i], a[5][3], k4[i], a[5][4], k5[i]), x[i]);
    rhs_int(m, y, u, k6);
    for (int i = 0; i < nx; ++i)
      ynew[i] = axpy(h, lc6(a[6][0], k1[i], a[6][1], k2[i], a[6][2], k3[i], a[6][3], k4[i], a[6][4], k5[i], a[6][5], k6[i]), x[i]);
    rhs_int(m, ynew, u, k7);
    for (int i = 0; i < nx; ++i)
      err[i] = h * lc7(e[0], k1[i], e[1], k2[i], e[2], k3[i], e[3], k4[i], e[4], k5[i], e[5], k6[i], e[6], k7[i]);
    double E = rms_scaled(err, x, ynew, nx, rtol, atol);
    if (E < 1.0) {
      double f = (E == 0.0) ? 10.0 : fmin(10.0, fmax(0.2, qtrunc6(0.9 * pow(E, -0.2))));
      if (rejected_last && f > 1.0) f = 1.0;
      t += h;
      h *= f;
      for (int i = 0; i < nx; ++i) { x[i] = ynew[i]; k1[i] = k7[i]; }
      rejected_last = 0;
      ++acc;
      if (last) break;
    } else {
      double f = (E == E) ? fmax(0.2, qtrunc6(0.9 * pow(E, -0.2))) : 0.2;
      if (f > 1.0) f = 1.0;
      h *= f;
      rejected_last = 1;
      ++rej;
      if (!(h > 1e-13 * dt)) { status = 2; break; }
    }
  }
  if (nacc) *nacc = acc;
  if (nrej) *nrej = rej;
  if (status != 0)
    for (int i = 0; i < nx; ++i) x[i] = NAN;
  return status;
}

/* Guarded fixed-step Tsit5 (PCG_INT_T5G, the cstr's default since round 3): nsub steps of the Tsit5 solution weights.
 * A step is TRUSTED when (i) the model's guard holds at its start state and at its end state (no growing mode, fastest
 * rate resolved: the guard shares the Arrhenius factor with the right-hand side; round 3 also evaluated it at the five
 * inner stage states -- with the estimate in place that changes no decision on 600,000 loop, 300,000 wide-box and 190,000
 * full-box env steps, and costs a sixth of the step's instructions) and -- round 4 -- (ii) Tsit5's own embedded
 * 5(4) error estimate of EVERY step stays below T5G_EST_TOL (mixed absolute / relative, RMS: the norm of the adaptive
 * pairs).  The estimate needs the seventh stage k7 = f(x_new); that evaluation IS the next step's first stage (FSAL) and
 * the end-state guard, so it costs the weights only.  (Round 3 accepted on the guard alone: outside the calibrated box --
 * a wider action box, a nearly burnt-out hot state -- the guard passed steps that were 4e-4 ... 6e-3 off)
 * Otherwise the adaptive explicit pair from the start state at the PLAN's tolerance (round 3 loosened it to 1e-7 on
 * contracting states without saying so in the header).  nacc = nrej = 0 marks a trusted env.
 * Twin of t5_guarded() / guarded_env() in pc-gym_amd/csrc. */
#define T5G_SLOW_LIMIT 2.0
static double g_t5g_est_tol = 4e-7; /* T5G_EST_TOL; orc_set_t5g_est_tol() is the calibration hook of tests/test_erk.py */
static double g_t5g_est_atol = 4e-9;
ORC_EXPORT void orc_set_t5g_est_tol(double v) { g_t5g_est_tol = v; g_t5g_est_atol = v; }
ORC_EXPORT void orc_set_t5g_est_tols(double rt, double at) { g_t5g_est_tol = rt; g_t5g_est_atol = at; }
static int t5g(const orc_model* m, double* x, const double* u, double dt, int nsub, double rtol, double atol, int max_steps,
               int32_t* nacc, int32_t* nrej) {
  int nx = m->nx;
  const double(*a)[6] = T5_A;
  const double* e = T5_E;
  double h = dt / nsub;
  double x0[MAXNX], k1[MAXNX], k2[MAXNX], k3[MAXNX], k4[MAXNX], k5[MAXNX], k6[MAXNX], k7[MAXNX], y[MAXNX], xn[MAXNX], err[MAXNX];
  int calm = 1, slow = 1, sharp = 1;
  for (int i = 0; i < nx; ++i) x0[i] = x[i];
  guard_ok(m, x, h, T5G_SLOW_LIMIT, &calm, &slow);
  rhs_int(m, x, u, k1);
  for (int s = 0; s < nsub; ++s) {
    for (int i = 0; i < nx; ++i) y[i] = axpy(h, lc1(a[1][0], k1[i]), x[i]);
    rhs_int(m, y, u, k2);
    for (int i = 0; i < nx; ++i) y[i] = axpy(h, lc2(a[2][0], k1[i], a[2][1], k2[i]), x[i]);
    rhs_int(m, y, u, k3);
    for (int i = 0; i < nx; ++i) y[i] = axpy(h, lc3(a[3][0], k1[i], a[3][1], k2[i], a[3][2], k3[i]), x[i]);
    rhs_int(m, y, u, k4);
    for (int i = 0; i < nx; ++i) y[i] = axpy(h, lc4(a[4][0], k1[i], a[4][1], k2[i], a[4][2], k3[i], a[4][3], k4[i]), x[i]);
    rhs_int(m, y, u, k5);
    for (int i = 0; i < nx; ++i)
      y[i] = axpy(h, lc5(a[5][0], k1[i], a[5][1], k2[i], a[5][2], k3[i], a[5][3], k4[i], a[5][4], k5[i]), x[i]);
    rhs_int(m, y, u, k6);
    for (int i = 0; i < nx; ++i)
      xn[i] = axpy(h, lc6(a[6][0], k1[i], a[6][1], k2[i], a[6][2], k3[i], a[6][3], k4[i], a[6][4], k5[i], a[6][5], k6[i]), x[i]);
    guard_ok(m, xn, h, T5G_SLOW_LIMIT, &calm, &slow); /* the step's end state = the next step's first stage state */
    rhs_int(m, xn, u, k7);
    for (int i = 0; i < nx; ++i)
      err[i] = h * lc7(e[0], k1[i], e[1], k2[i], e[2], k3[i], e[3], k4[i], e[4], k5[i], e[5], k6[i], e[6], k7[i]);
    { /* mean over the components of (err_i / sc_i)^2 < 1, sc_i = atol + rtol max(|x_i|, |xn_i|) (NaN fails); for two
       * states written without divisions -- err_0^2 sc_1^2 + err_1^2 sc_0^2 < 2 sc_0^2 sc_1^2 -- as the kernel does */
      double e2[MAXNX], c2[MAXNX];
      for (int i = 0; i < nx; ++i) {
        double a0 = fabs(x[i]), a1 = fabs(xn[i]);
        double sc = g_t5g_est_atol + g_t5g_est_tol * (a0 > a1 ? a0 : a1);
        e2[i] = err[i] * err[i];
        c2[i] = sc * sc;
      }
      int ok;
      if (nx == 2) ok = (e2[0] * c2[1] + e2[1] * c2[0]) < 2.0 * (c2[0] * c2[1]);
      else {
        double s2 = 0.0;
        for (int i = 0; i < nx; ++i) s2 += e2[i] / c2[i];
        ok = s2 * (1.0 / nx) < 1.0;
      }
      if (!ok) sharp = 0;
    }
    for (int i = 0; i < nx; ++i) { x[i] = xn[i]; k1[i] = k7[i]; }
  }
  if (nacc) *nacc = 0;
  if (nrej) *nrej = 0;
  if (calm && slow && sharp) return 0;
  for (int i = 0; i < nx; ++i) x[i] = x0[i];
  return dopri5(m, x, u, dt, rtol, atol, max_steps, nacc, nrej);
}

/* Cooper & Verner (1972) explicit Runge-Kutta method of order 8 in 11 stages, fixed step (PCG_INT_CV8): for smooth
 * right-hand sides ONE step per env step replaces five RK4 steps -- four_tank at the canonical dt: 7.2e-7 of a 1e-13
 * solve with 11 evaluations against 1.8e-6 with 20 (tools/prototypes/erk_fixed.py).  Coefficients in sqrt(21), written
 * as correctly rounded doubles; pinned by the order conditions in tests/test_erk.py.  Twin of cv8() in
 * pc-gym_amd/csrc/pcg_integrators.hpp: every stage sum is a chain of fused multiply-adds over the non-zero
 * coefficients in increasing stage order, then one fma with h. */
static const double CV8_A[11][10] = {
    {0},
    {0.5},
    {0.25, 0.25},
    {0.14285714285714285, -0.2117115008659951, 0.8961811933628409},
    {0.18550685351137905, 0, 0.5766714726956089, 0.06514850914700064},
    {0.19963699364491333, 0, 0.3772937693043289, -0.46345538964060623, 0.386524626691364},
    {0.1289862929772419, 0, -0.03302551131448482, -0.3497052863177422, 0.32851721314173715, 0.09790045615925942},
    {0.07142857142857142, 0, 0, 0, 0.0020021659931149204, -0.011868683886786031, 0.1111111111111111},
    {0.03125, 0, 0, 0, -0.009086961100820556, 0.1527777777777778, -0.6325461606959097, 0.9576053440189525},
    {0.07142857142857142, 0, 0, 0, 0.1111111111111111, -0.6379313501852646, 2.031083139166862, -1.8108630829377543,
     1.0624984467704635},
    {0, 0, 0, 0, -0.5512205630727289, 2.451380432416967, -7.164951553231382, 7.553840442120271, -2.2291582101947447,
     0.9401094519616178}};
static const double CV8_B[11] = {0.05, 0, 0, 0, 0, 0, 0, 0.2722222222222222, 0.35555555555555557, 0.2722222222222222, 0.05};
ORC_EXPORT void orc_cv8_tableau(double* a110, double* b11) {
  memcpy(a110, CV8_A, sizeof CV8_A);
  memcpy(b11, CV8_B, sizeof CV8_B);
}
static void cv8(const orc_model* m, double* x, const double* u, double dt, int nsub) {
  int nx = m->nx;
  double h = dt / nsub;
  double k[11][MAXNX], y[MAXNX];
  for (int s = 0; s < nsub; ++s) {
    rhs_int(m, x, u, k[0]);
    for (int st = 1; st < 11; ++st) {
      for (int i = 0; i < nx; ++i) {
        double acc = 0.0;
        int first = 1;
        for (int j = 0; j < st; ++j) {
          if (CV8_A[st][j] == 0.0) continue;
          acc = first ? CV8_A[st][j] * k[j][i] : fma(CV8_A[st][j], k[j][i], acc);
          first = 0;
        }
        y[i] = fma(h, acc, x[i]);
      }
      rhs_int(m, y, u, k[st]);
    }
    for (int i = 0; i < nx; ++i) {
      double acc = CV8_B[0] * k[0][i];
      for (int j = 7; j < 11; ++j) acc = fma(CV8_B[j], k[j][i], acc);
      x[i] = fma(h, acc, x[i]);
    }
  }
}

/* Rodas3 (Sandu et al. 1997): 4-stage linearly implicit Rosenbrock 3(2) pair, gamma = 1/2, L-stable, stiffly accurate
 * -- the stiff-capable integrator of the engine (the reference solves with CVODES BDF, integrator.py:163-182; its
 * recorded LSODA trajectories are the accuracy pin, tests/test_oracle_golden.py).  Twin of rodas3() in
 * pc-gym_amd/csrc/pcg_integrators.hpp, statement by statement: forward-difference Jacobian, W = I/(gamma h) - J, LU with
 * partial pivoting, four solves; error = the fourth stage increment; factor = clip(Q(0.9 E^-1/3), 0.2, 6). */
static int ros_lu(double* W, int* piv, int n) {
  int ok = 1;
  for (int k = 0; k < n; ++k) {
    int pk = k;
    double best = fabs(W[k * n + k]);
    for (int i = k + 1; i < n; ++i) {
      double v = fabs(W[i * n + k]);
      if (v > best) { best = v; pk = i; }
    }
    piv[k] = pk;
    for (int j = 0; j < n; ++j) { double a = W[k * n + j]; W[k * n + j] = W[pk * n + j]; W[pk * n + j] = a; }
    double d = W[k * n + k];
    ok = ok && (fabs(d) > 1e-300) && (d == d);
    double inv = 1.0 / d;
    for (int i = k + 1; i < n; ++i) {
      double l = W[i * n + k] * inv;
      W[i * n + k] = l;
      for (int j = k + 1; j < n; ++j) W[i * n + j] = W[i * n + j] - l * W[k * n + j];
    }
  }
  return ok;
}
static void ros_solve(const double* W, const int* piv, int n, double* b) {
  for (int k = 0; k < n; ++k) { double a = b[k]; b[k] = b[piv[k]]; b[piv[k]] = a; }
  for (int i = 1; i < n; ++i) {
    double sacc = b[i];
    for (int j = 0; j < i; ++j) sacc -= W[i * n + j] * b[j];
    b[i] = sacc;
  }
  for (int i = n - 1; i >= 0; --i) {
    double sacc = b[i];
    for (int j = i + 1; j < n; ++j) sacc -= W[i * n + j] * b[j];
    b[i] = sacc / W[i * n + i];
  }
}
static double ros_factor(double E) { return qtrunc6(0.9 * pow(E, -1.0 / 3.0)); }

static int rodas3(const orc_model* m, double* x, const double* u, double dt, double rtol, double atol,
                  int max_steps, int32_t* nacc, int32_t* nrej) {
  const double gam = 0.5;
  int n = m->nx;
  double f0[MAXNX], k1[MAXNX], k2[MAXNX], k3[MAXNX], k4[MAXNX], y[MAXNX], fy[MAXNX];
  double* W = (double*)malloc(sizeof(double) * (size_t)n * n);
  int piv[MAXNX];
  int acc = 0, rej = 0, status = 0;
  rhs_int(m, x, u, f0);
  double h;
  {
    double d0 = rms_scaled(x, x, x, n, rtol, atol);
    double d1 = rms_scaled(f0, x, x, n, rtol, atol);
    double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    h = fmin(qtrunc6(100.0 * h0), dt);
  }
  double t = 0.0;
  int rejected_last = 0;
  for (;;) {
    int last = 0;
    if (acc + rej >= max_steps) { status = 1; break; }
    if (t + h >= dt * (1.0 - 1e-14)) { h = dt - t; last = 1; }
    /* perturbation ~ sqrt(eps) / rtol x the error weight of the component, atol + rtol |x_j| (CVODES' difference
     * quotient scales the same way); the x_max term only keeps it non-zero when atol = 0 and x_j = 0 */
    double xmax = 0.0;
    for (int i = 0; i < n; ++i) xmax = fmax(xmax, fabs(x[i]));
    const double wfloor = atol / rtol + 1e-12 * xmax + 1e-100;
    for (int j = 0; j < n; ++j) {
      double xj = x[j];
      double del = 1.4901161193847656e-8 * (fabs(xj) + wfloor);
      for (int i = 0; i < n; ++i) y[i] = x[i];
      y[j] = xj + del;
      rhs_int(m, y, u, fy);
      double idel = 1.0 / ((xj + del) - xj);
      for (int i = 0; i < n; ++i) W[i * n + j] = -(fy[i] - f0[i]) * idel;
    }
    double igh = 1.0 / (gam * h), ih = 1.0 / h;
    for (int i = 0; i < n; ++i) W[i * n + i] = W[i * n + i] + igh;
    int lu_ok = ros_lu(W, piv, n);
    for (int i = 0; i < n; ++i) k1[i] = f0[i];
    ros_solve(W, piv, n, k1);
    for (int i = 0; i < n; ++i) k2[i] = f0[i] + (4.0 * ih) * k1[i];
    ros_solve(W, piv, n, k2);
    for (int i = 0; i < n; ++i) y[i] = x[i] + 2.0 * k1[i];
    rhs_int(m, y, u, fy);
    for (int i = 0; i < n; ++i) k3[i] = fy[i] + ih * (k1[i] - k2[i]);
    ros_solve(W, piv, n, k3);
    for (int i = 0; i < n; ++i) y[i] = x[i] + 2.0 * k1[i] + k3[i];
    rhs_int(m, y, u, fy);
    for (int i = 0; i < n; ++i) k4[i] = fy[i] + ih * (k1[i] - k2[i] - (8.0 / 3.0) * k3[i]);
    ros_solve(W, piv, n, k4);
    for (int i = 0; i < n; ++i) y[i] = x[i] + 2.0 * k1[i] + k3[i] + k4[i];
    double E = rms_scaled(k4, x, y, n, rtol, atol);
    if (!lu_ok) E = NAN;
    if (E < 1.0) {
      double f = (E == 0.0) ? 6.0 : fmin(6.0, fmax(0.2, ros_factor(E)));
      if (rejected_last && f > 1.0) f = 1.0;
      t += h;
      h *= f;
      for (int i = 0; i < n; ++i) x[i] = y[i];
      rejected_last = 0;
      ++acc;
      if (last) break;
      rhs_int(m, x, u, f0);
    } else {
      double f = (E == E) ? fmax(0.2, ros_factor(E)) : 0.2;
      if (f > 1.0) f = 1.0;
      h *= f;
      rejected_last = 1;
      ++rej;
      if (!(h > 1e-13 * dt)) { status = 2; break; }
    }
  }
  free(W);
  if (nacc) *nacc = acc;
  if (nrej) *nrej = rej;
  if (status != 0)
    for (int i = 0; i < n; ++i) x[i] = NAN;
  return status;
}

/* ---------------------------------------------------------------------------------------------------------------
 * Rodas4 (Hairer & Wanner, "Solving ODEs II", RODAS with the coefficient set of their code's METH = 1): 6-stage
 * linearly implicit Rosenbrock 4(3) pair, gamma = 1/4, L-stable, stiffly accurate; in the transformed form
 *     (I/(gamma h) - J) U_i = f(x + sum_j a_ij U_j) + sum_j (c_ij / h) U_j,   x_new = y_6 + U_6,   error = U_6
 * with y_5 = x + sum a_5j U_j and y_6 = y_5 + U_5.  The eight order-4 conditions hold for this tableau to 2e-15
 * (tests/test_oracle_golden.py re-derives (alpha, Gamma, b) from (a, C, m) and checks them).  Twin of rodas4() in
 * pc-gym_amd/csrc/pcg_integrators.hpp, statement by statement (this file is compiled with -ffp-contract=off, fma()
 * where the kernel has an fma).
 *   linear algebra   the 10-state extraction cascade has an analytic Jacobian with two interleaved bidiagonal chains
 *                    (X couples down the cascade, Y up, and the mass transfer couples X_s with Y_s): in the natural
 *                    order (X1,Y1,X2,Y2,...) W is banded and an M-matrix for Y >= 0, so it is eliminated without
 *                    pivoting -- me_ros_factor / me_ros_solve below: one reciprocal for all five X pivots, one per Y
 *                    pivot, ~33 flops per solve.  Every other model: forward-difference Jacobian + the dense pivoted
 *                    LU of Rodas3.
 *   controller       RMS norm, accept iff E < 1, factor = clip(Q(0.9 E^-1/4), 0.2, 6) (<= 1 right after a rejection),
 *                    first step min(Q(5 h0), dt) with Hairer's h0, same failure semantics as dopri5 / rodas3.
 *   end-point error control (cfg.ep_kmax > 0, models with a contraction rate mu(u) > 0): an env step hands only
 *                    x(dt) on; an error committed at time t' reaches it damped by ~exp(-mu (dt - t')), so the tolerance
 *                    of the attempt that ends at t' is multiplied by 2^k, k = min(ep_kmax, trunc(ep_frac log2(e) mu
 *                    (dt - t'))) -- E2 is scaled by the exact power of two 4^-k.
 * ------------------------------------------------------------------------------------------------------------- */
static const double R4_GAM = 0.25;
static const double R4_A21 = 0.1544000000000000e+01, R4_A31 = 0.9466785280815826e+00, R4_A32 = 0.2557011698983284e+00,
                    R4_A41 = 0.3314825187068521e+01, R4_A42 = 0.2896124015972201e+01, R4_A43 = 0.9986419139977817e+00,
                    R4_A51 = 0.1221224509226641e+01, R4_A52 = 0.6019134481288629e+01, R4_A53 = 0.1253708332932087e+02,
                    R4_A54 = -0.6878860361058950e+00;
static const double R4_C21 = -0.5668800000000000e+01, R4_C31 = -0.2430093356833875e+01, R4_C32 = -0.2063599157091915e+00,
                    R4_C41 = -0.1073529058151375e+00, R4_C42 = -0.9594562251023355e+01, R4_C43 = -0.2047028614809616e+02,
                    R4_C51 = 0.7496443313967647e+01, R4_C52 = -0.1024680431464352e+02, R4_C53 = -0.3399990352819905e+02,
                    R4_C54 = 0.1170890893206160e+02, R4_C61 = 0.8083246795921522e+01, R4_C62 = -0.7981132988064893e+01,
                    R4_C63 = -0.3152159432874371e+02, R4_C64 = 0.1631930543123136e+02, R4_C65 = -0.6058818238834054e+01;
ORC_EXPORT void orc_rodas4_tableau(double* a15, double* c15, double* gam) {
  const double a[10] = {R4_A21, R4_A31, R4_A32, R4_A41, R4_A42, R4_A43, R4_A51, R4_A52, R4_A53, R4_A54};
  const double c[15] = {R4_C21, R4_C31, R4_C32, R4_C41, R4_C42, R4_C43, R4_C51, R4_C52, R4_C53, R4_C54,
                        R4_C61, R4_C62, R4_C63, R4_C64, R4_C65};
  memcpy(a15, a, sizeof a);
  memcpy(c15, c, sizeof c);
  *gam = R4_GAM;
}

/* End-point exponents of the two component groups of a model at time-to-go tau (twin of M::ep_exponents):
 *   extraction cascades: a perturbation decays with the slower of the two through-flow rates, a = L/Vl (liquid chain)
 *   and c = G/Vg (gas chain) -- k_s = trunc(min(kmax, ep_c min(a,c) tau)) for every component.  The 10-state model
 *   splits further: group 0 = liquid (X), group 1 = gas (Y).  An error in the FAST chain dies at its own rate and only
 *   reaches the slow chain through the mass-transfer coupling, attenuated by (coupling rate x residence time):
 *   kappa/c for Y -> X (kappa = Kla 2 Ymax / m, Ymax = 1: the top of the observation box) and e/(a + Kla) for X -> Y
 *   (e = Kla Vl/Vg); with a safety factor 2:  k_Y = min(kmax, trunc(ep_c c tau), k_s + floor(log2(max(1, c/(2 kappa))))),
 *   k_X likewise.  The logarithms are exponent extractions: exact.
 *   other models: 0 (classical local error control). */
static int ep_trunc(double v, int kmax) { return (v > 0.0) ? (int)fmin(v, (double)kmax) : 0; }
static int ep_ilog2(double v) { /* floor(log2(v)) for v >= 1, 0 below */
  int e;
  if (!(v >= 1.0)) return 0;
  frexp(v, &e);
  return e - 1;
}
static void ep_exponents(const orc_model* m, const double* u, double ep_c, int kmax, double tau, int* kg) {
  kg[0] = kg[1] = 0;
  if (kmax <= 0) return;
  if (m->model_id == PCG_MODEL_ME || m->model_id == PCG_MODEL_ME_REACTIVE) {
    const double iVl = 1 / m->p[0], iVg = 1 / m->p[1];
    const double a = u[0] * iVl, c = u[1] * iVg;
    const double ct = ep_c * tau;
    const int ks = ep_trunc(ct * fmin(a, c), kmax);
    kg[0] = kg[1] = ks;
    if (m->model_id == PCG_MODEL_ME && m->p[4] == 2.0) { /* the coupling bound is the slope of the eq_exponent == 2 curve */
      const double inv_m = 1 / m->p[2], KlaVl = m->p[3] * m->p[0];
      const double klap = iVl * KlaVl, e = iVg * KlaVl;
      const double kappa2 = (klap * 2.0 * inv_m) * 2.0, e2 = e * 2.0; /* x safety 2 */
      const int kX = ks + ep_ilog2((a + klap) / e2), kY = ks + ep_ilog2(c / kappa2);
      const int kXd = ep_trunc(ct * a, kmax), kYd = ep_trunc(ct * c, kmax);
      kg[0] = kX < kXd ? kX : kXd;
      kg[1] = kY < kYd ? kY : kYd;
    }
  }
}
static int ep_group(const orc_model* m, int i) { return (m->model_id == PCG_MODEL_ME) ? (i & 1) : 0; }

/* W = theta I - J of the 10-state extraction model (kernel-order constants), eliminated in the natural order
 * (X1,Y1,...,X5,Y5) without pivoting.  Rows:  X_s:  DX X_s - alpha X_{s-1} - cx_s Y_s ;  Y_s:  -e X_s + DY_s Y_s - beta Y_{s+1}
 * with alpha = L/Vl, beta = G/Vg, e = Kla Vl/Vg, q_s = d(Y^ex/m)/dY, cx_s = Kla q_s, DX = theta + alpha + Kla,
 * DY_s = theta + beta + e q_s.  The X pivots stay DX; fill-in only at (X_{s+1}, Y_s). */
typedef struct {
  double iDX, aD, eD, beta;
  double ct[5], iDY[5], m3[4];
  int ok;
} me_ros_fac;
static void me_ros_factor(const double* p, const double* u, const double* x, double theta, me_ros_fac* F) {
  const double iVl = 1 / p[0], iVg = 1 / p[1], inv_m = 1 / p[2], KlaVl = p[3] * p[0], ex = p[4];
  const double alpha = u[0] * iVl, beta = u[1] * iVg, klap = iVl * KlaVl, e = iVg * KlaVl;
  const double DX = theta + (alpha + klap);
  const double thb = theta + beta;
  F->iDX = 1.0 / DX;
  F->aD = alpha * F->iDX;
  F->eD = e * F->iDX;
  F->beta = beta;
  int ok = (DX > 0.0) && (DX < INFINITY);
  double ct = 0.0;
  for (int s = 0; s < 5; ++s) {
    const double Y = x[2 * s + 1];
    const double q = (ex == 2.0) ? (2.0 * Y) * inv_m : (ex * pow(Y, ex - 1.0)) * inv_m;
    const double cx = klap * q;
    ct = (s == 0) ? cx : fma(F->m3[s - 1], beta, cx);
    const double DY = fma(e, q, thb);
    const double DYp = fma(-F->eD, ct, DY);
    ok = ok && (DYp > 0.0) && (DYp < INFINITY);
    F->ct[s] = ct;
    F->iDY[s] = 1.0 / DYp;
    if (s < 4) F->m3[s] = (F->aD * ct) * F->iDY[s];
  }
  F->ok = ok;
}
static void me_ros_solve(const me_ros_fac* F, double* b) {
  for (int s = 0; s < 5; ++s) {
    b[2 * s + 1] = fma(F->eD, b[2 * s], b[2 * s + 1]);
    if (s < 4) {
      b[2 * s + 2] = fma(F->aD, b[2 * s], b[2 * s + 2]);
      b[2 * s + 2] = fma(F->m3[s], b[2 * s + 1], b[2 * s + 2]);
    }
  }
  for (int s = 4; s >= 0; --s) {
    const double yv = ((s == 4) ? b[2 * s + 1] : fma(F->beta, b[2 * s + 3], b[2 * s + 1])) * F->iDY[s];
    b[2 * s + 1] = yv;
    b[2 * s] = fma(F->ct[s], yv, b[2 * s]) * F->iDX;
  }
}
/* test hook: z = W^-1 b through the structured elimination (tests compare with a dense solve of theta I - J_fd) */
ORC_EXPORT int orc_me_ros_solve(const double* p, const double* u, const double* x, double theta, double* b) {
  me_ros_fac F;
  me_ros_factor(p, u, x, theta, &F);
  me_ros_solve(&F, b);
  return F.ok;
}

static int g_ros4_structured = 1; /* test switch: 0 = dense finite-difference path for every model */
/* calibration hook of the pair's controller (tools/prototypes): first step x h0, safety, largest growth, smallest factor */
static double g_r4_h0 = 5.0, g_r4_safety = 0.9, g_r4_facmax = 6.0, g_r4_facmin = 0.2;
ORC_EXPORT void orc_set_rodas4_ctrl(double h0, double safety, double facmax, double facmin) {
  g_r4_h0 = h0; g_r4_safety = safety; g_r4_facmax = facmax; g_r4_facmin = facmin;
}
ORC_EXPORT void orc_set_ros4_structured(int on) { g_ros4_structured = on; }

static int rodas4(const orc_model* m, double* x, const double* u, double dt, double rtol, double atol, int max_steps,
                  double ep_frac, int ep_kmax, int32_t* nacc, int32_t* nrej) {
  int n = m->nx;
  const int structured = g_ros4_structured && m->model_id == PCG_MODEL_ME;
  double f0[MAXNX], U1[MAXNX], U2[MAXNX], U3[MAXNX], U4[MAXNX], U5[MAXNX], U6[MAXNX], y[MAXNX], fy[MAXNX], r[MAXNX];
  double* W = structured ? 0 : (double*)malloc(sizeof(double) * (size_t)n * n);
  int piv[MAXNX];
  me_ros_fac F;
  int acc = 0, rej = 0, status = 0;
  rhs_int(m, x, u, f0);
  double h;
  {
    double d0 = rms_scaled(x, x, x, n, rtol, atol);
    double d1 = rms_scaled(f0, x, x, n, rtol, atol);
    double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    /* 5 h0: measured over the action box of BASELINE configs[2], 100 h0 (Rodas3's choice) costs 3.9 rejected attempts
     * per env step out of 22.5, 5 h0 costs 0.5 out of 19.6 at the same worst-case error */
    h = fmin(qtrunc6(g_r4_h0 * h0), dt);
  }
  /* end-point error control: exponent rate per unit of contraction rate, in bits */
  const double ep_c = (ep_kmax > 0) ? ep_frac * 1.4426950408889634 : 0.0;
  double t = 0.0;
  int rejected_last = 0;
  for (;;) {
    int last = 0;
    if (acc + rej >= max_steps) { status = 1; break; }
    if (t + h >= dt * (1.0 - 1e-14)) { h = dt - t; last = 1; }
    const double igh = 1.0 / (R4_GAM * h), ih = 1.0 / h;
    int lu_ok;
    if (structured) {
      me_ros_factor(m->p, u, x, igh, &F);
      lu_ok = F.ok;
    } else {
      double xmax = 0.0;
      for (int i = 0; i < n; ++i) xmax = fmax(xmax, fabs(x[i]));
      const double wfloor = atol / rtol + 1e-12 * xmax + 1e-100;
      for (int j = 0; j < n; ++j) {
        double xj = x[j];
        double del = 1.4901161193847656e-8 * (fabs(xj) + wfloor);
        for (int i = 0; i < n; ++i) y[i] = x[i];
        y[j] = xj + del;
        rhs_int(m, y, u, fy);
        double idel = 1.0 / ((xj + del) - xj);
        for (int i = 0; i < n; ++i) W[i * n + j] = -(fy[i] - f0[i]) * idel;
      }
      for (int i = 0; i < n; ++i) W[i * n + i] = W[i * n + i] + igh;
      lu_ok = ros_lu(W, piv, n);
    }
#define R4_SOLVE(v) do { if (structured) me_ros_solve(&F, v); else ros_solve(W, piv, n, v); } while (0)
    const double c21 = R4_C21 * ih, c31 = R4_C31 * ih, c32 = R4_C32 * ih, c41 = R4_C41 * ih, c42 = R4_C42 * ih,
                 c43 = R4_C43 * ih, c51 = R4_C51 * ih, c52 = R4_C52 * ih, c53 = R4_C53 * ih, c54 = R4_C54 * ih,
                 c61 = R4_C61 * ih, c62 = R4_C62 * ih, c63 = R4_C63 * ih, c64 = R4_C64 * ih, c65 = R4_C65 * ih;
    for (int i = 0; i < n; ++i) U1[i] = f0[i];
    R4_SOLVE(U1);
    for (int i = 0; i < n; ++i) y[i] = fma(R4_A21, U1[i], x[i]);
    rhs_int(m, y, u, fy);
    for (int i = 0; i < n; ++i) U2[i] = fma(c21, U1[i], fy[i]);
    R4_SOLVE(U2);
    for (int i = 0; i < n; ++i) y[i] = fma(R4_A32, U2[i], fma(R4_A31, U1[i], x[i]));
    rhs_int(m, y, u, fy);
    for (int i = 0; i < n; ++i) U3[i] = fma(c32, U2[i], fma(c31, U1[i], fy[i]));
    R4_SOLVE(U3);
    for (int i = 0; i < n; ++i) y[i] = fma(R4_A43, U3[i], fma(R4_A42, U2[i], fma(R4_A41, U1[i], x[i])));
    rhs_int(m, y, u, fy);
    for (int i = 0; i < n; ++i) U4[i] = fma(c43, U3[i], fma(c42, U2[i], fma(c41, U1[i], fy[i])));
    R4_SOLVE(U4);
    for (int i = 0; i < n; ++i)
      y[i] = fma(R4_A54, U4[i], fma(R4_A53, U3[i], fma(R4_A52, U2[i], fma(R4_A51, U1[i], x[i]))));
    rhs_int(m, y, u, fy);
    for (int i = 0; i < n; ++i) U5[i] = fma(c54, U4[i], fma(c53, U3[i], fma(c52, U2[i], fma(c51, U1[i], fy[i]))));
    R4_SOLVE(U5);
    for (int i = 0; i < n; ++i) y[i] = y[i] + U5[i];
    rhs_int(m, y, u, fy);
    for (int i = 0; i < n; ++i)
      U6[i] = fma(c65, U5[i], fma(c64, U4[i], fma(c63, U3[i], fma(c62, U2[i], fma(c61, U1[i], fy[i])))));
    R4_SOLVE(U6);
#undef R4_SOLVE
    for (int i = 0; i < n; ++i) r[i] = y[i] + U6[i]; /* the new solution; error = U6 */
    /* mean square of the scaled error, every term weighted by the end-point exponent of its component's group
     * (exact powers of two): accept iff E2 < 1 */
    int kg[2];
    ep_exponents(m, u, ep_c, ep_kmax, dt - (t + h), kg);
    const double sg[2] = {ldexp(1.0, -2 * kg[0]), ldexp(1.0, -2 * kg[1])};
    double E2 = 0.0;
    for (int i = 0; i < n; ++i) {
      double a0 = fabs(x[i]), a1 = fabs(r[i]);
      double q = U6[i] / (atol + rtol * (a0 > a1 ? a0 : a1));
      E2 += (q * q) * sg[ep_group(m, i)];
    }
    E2 = E2 * (1.0 / n);
    if (!lu_ok) E2 = NAN;
    if (E2 < 1.0) {
      double f = (E2 == 0.0) ? g_r4_facmax : fmin(g_r4_facmax, fmax(g_r4_facmin, qtrunc6(g_r4_safety * pow(E2, -0.125))));
      if (rejected_last && f > 1.0) f = 1.0;
      t += h;
      h *= f;
      for (int i = 0; i < n; ++i) x[i] = r[i];
      rejected_last = 0;
      ++acc;
      if (last) break;
      rhs_int(m, x, u, f0);
    } else {
      double f = (E2 == E2) ? fmax(g_r4_facmin, qtrunc6(g_r4_safety * pow(E2, -0.125))) : g_r4_facmin;
      if (f > 1.0) f = 1.0;
      h *= f;
      rejected_last = 1;
      ++rej;
      if (!(h > 1e-13 * dt)) { status = 2; break; }
    }
  }
  if (W) free(W);
  if (nacc) *nacc = acc;
  if (nrej) *nrej = rej;
  if (status != 0)
    for (int i = 0; i < n; ++i) x[i] = NAN;
  return status;
}

/* ---------------------------------------------------------------------------------------------------------------
 * Rodas5 (Di Marzo's coefficient set, the METH of Hairer & Wanner's RODAS5 code): 8-stage linearly implicit Rosenbrock
 * 5(4) pair, gamma = 0.19, L-stable, stiffly accurate, in the same transformed form as Rodas4 above:
 *     (I/(gamma h) - J) U_i = f(x + sum_j a_ij U_j) + sum_j (c_ij / h) U_j,
 *     y_7 = y_6 + U_6,  y_8 = y_7 + U_7,  x_new = y_8 + U_8,  error estimate = U_8 (against the embedded order-4 solution y_8).
 * The 17 order-5 conditions are checked by tests/test_rodas5.py (convergence order on a nonlinear problem, row sums,
 * quadrature conditions, stiff accuracy re-derived from (a, C)).  Linear algebra, error norm, end-point weights,
 * first step and failure semantics: rodas4's; factor = clip(Q(safety E^-1/5), facmin, facmax).
 * Twin of rodas5() in pc-gym_amd/csrc/pcg_integrators.hpp.
 * ------------------------------------------------------------------------------------------------------------- */
#define R5_S 8
static const double R5_GAM = 0.19;
static const double R5_A[6][5] = {
    {0, 0, 0, 0, 0},
    {2.0, 0, 0, 0, 0},
    {3.040894194418781, 1.041747909077569, 0, 0, 0},
    {2.576417536461461, 1.622083060776640, -0.9089668560264532, 0, 0},
    {2.760842080225597, 1.446624659844071, -0.3036980084553738, 0.2877498600325443, 0},
    {-14.09640773051259, 6.925207756232704, -41.47510893210728, 2.343771018586405, 24.13215229196062}};
static const double R5_C[8][7] = {
    {0, 0, 0, 0, 0, 0, 0},
    {-10.31323885133993, 0, 0, 0, 0, 0, 0},
    {-21.04823117650003, -7.234992135176716, 0, 0, 0, 0, 0},
    {32.22751541853323, -4.943732386540191, 19.44922031041879, 0, 0, 0, 0},
    {-20.69865579590063, -8.816374604402768, 1.260436877740897, -0.7495647613787146, 0, 0, 0},
    {-46.22004352711257, -17.49534862857472, -289.6389582892057, 93.60855400400906, 318.3822534212147, 0, 0},
    {34.20013733472935, -14.15535402717690, 57.82335640988400, 25.83362985412365, 1.408950972071624, -6.551835421242162, 0},
    {42.57076742291101, -13.80770672017997, 93.98938432427124, 18.77919633714503, -31.58359187223370, -6.685968952921985,
     -5.810979938412932}};
ORC_EXPORT void orc_rodas5_tableau(double* a15, double* c28, double* gam) {
  int k = 0;
  for (int i = 1; i < 6; ++i)
    for (int j = 0; j < i; ++j) a15[k++] = R5_A[i][j];
  k = 0;
  for (int i = 1; i < 8; ++i)
    for (int j = 0; j < i; ++j) c28[k++] = R5_C[i][j];
  *gam = R5_GAM;
}
static double g_r5_h0 = 10.0, g_r5_safety = 0.9, g_r5_facmax = 6.0, g_r5_facmin = 0.2; /* (calibration hook below; r5::H0 of the kernels) */
static double g_r5_hcap = 2.0;
ORC_EXPORT void orc_set_rodas5_hcap(double kb) { g_r5_hcap = kb; }
ORC_EXPORT void orc_set_rodas5_ctrl(double h0, double safety, double facmax, double facmin) {
  g_r5_h0 = h0; g_r5_safety = safety; g_r5_facmax = facmax; g_r5_facmin = facmin;
}
static int rodas5(const orc_model* m, double* x, const double* u, double dt, double rtol, double atol, int max_steps,
                  double ep_frac, int ep_kmax, int32_t* nacc, int32_t* nrej) {
  int n = m->nx;
  const int structured = g_ros4_structured && m->model_id == PCG_MODEL_ME;
  double f0[MAXNX], U[R5_S][MAXNX], y[MAXNX], fy[MAXNX], r[MAXNX];
  double* W = structured ? 0 : (double*)malloc(sizeof(double) * (size_t)n * n);
  int piv[MAXNX];
  me_ros_fac F;
  int acc = 0, rej = 0, status = 0;
  rhs_int(m, x, u, f0);
  double h;
  {
    double d0 = rms_scaled(x, x, x, n, rtol, atol);
    double d1 = rms_scaled(f0, x, x, n, rtol, atol);
    double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    h = fmin(qtrunc6(g_r5_h0 * h0), dt);
  }
  const double ep_c = (ep_kmax > 0) ? ep_frac * 1.4426950408889634 : 0.0;
  double t = 0.0;
  int rejected_last = 0;
  for (;;) {
    int last = 0;
    if (acc + rej >= max_steps) { status = 1; break; }
    if (t + h >= dt * (1.0 - 1e-14)) { h = dt - t; last = 1; }
    const double ih = 1.0 / h, igh = ih * (1.0 / R5_GAM);
    int lu_ok;
    if (structured) {
      me_ros_factor(m->p, u, x, igh, &F);
      lu_ok = F.ok;
    } else {
      double xmax = 0.0;
      for (int i = 0; i < n; ++i) xmax = fmax(xmax, fabs(x[i]));
      const double wfloor = atol / rtol + 1e-12 * xmax + 1e-100;
      for (int j = 0; j < n; ++j) {
        double xj = x[j];
        double del = 1.4901161193847656e-8 * (fabs(xj) + wfloor);
        for (int i = 0; i < n; ++i) y[i] = x[i];
        y[j] = xj + del;
        rhs_int(m, y, u, fy);
        double idel = 1.0 / ((xj + del) - xj);
        for (int i = 0; i < n; ++i) W[i * n + j] = -(fy[i] - f0[i]) * idel;
      }
      for (int i = 0; i < n; ++i) W[i * n + i] = W[i * n + i] + igh;
      lu_ok = ros_lu(W, piv, n);
    }
    for (int s = 0; s < R5_S; ++s) {
      if (s == 0) {
        for (int i = 0; i < n; ++i) U[0][i] = f0[i];
      } else {
        if (s < 6) { /* y = x + sum_j a_sj U_j, innermost term j = 0 */
          for (int i = 0; i < n; ++i) {
            double v = x[i];
            for (int j = 0; j < s; ++j) v = fma(R5_A[s][j], U[j][i], v);
            y[i] = v;
          }
        } else {
          for (int i = 0; i < n; ++i) y[i] = y[i] + U[s - 1][i];
        }
        rhs_int(m, y, u, fy);
        for (int i = 0; i < n; ++i) {
          double v = fy[i];
          for (int j = 0; j < s; ++j) v = fma(R5_C[s][j] * ih, U[j][i], v);
          U[s][i] = v;
        }
      }
      if (structured) me_ros_solve(&F, U[s]); else ros_solve(W, piv, n, U[s]);
    }
    for (int i = 0; i < n; ++i) r[i] = y[i] + U[7][i]; /* the new solution; error = U8 */
    int kg[2];
    ep_exponents(m, u, ep_c, ep_kmax, dt - (t + h), kg);
    if (g_r5_hcap > 0.0) { /* see ros_pair() in pcg_integrators.hpp */
      const int kc = ep_trunc(g_r5_hcap * ((dt - (t + h)) * ih), 1000);
      if (kg[0] > kc) kg[0] = kc;
      if (kg[1] > kc) kg[1] = kc;
    }
    const double sg[2] = {ldexp(1.0, -2 * kg[0]), ldexp(1.0, -2 * kg[1])};
    double E2 = 0.0;
    for (int i = 0; i < n; ++i) {
      double a0 = fabs(x[i]), a1 = fabs(r[i]);
      double q = U[7][i] / (atol + rtol * (a0 > a1 ? a0 : a1));
      E2 += (q * q) * sg[ep_group(m, i)];
    }
    E2 = E2 * (1.0 / n);
    if (!lu_ok) E2 = NAN;
    if (E2 < 1.0) {
      double f = (E2 == 0.0) ? g_r5_facmax : fmin(g_r5_facmax, fmax(g_r5_facmin, qtrunc6(g_r5_safety * pow(E2, -0.1))));
      if (rejected_last && f > 1.0) f = 1.0;
      t += h;
      h *= f;
      for (int i = 0; i < n; ++i) x[i] = r[i];
      rejected_last = 0;
      ++acc;
      if (last) break;
      rhs_int(m, x, u, f0);
    } else {
      double f = (E2 == E2) ? fmax(g_r5_facmin, qtrunc6(g_r5_safety * pow(E2, -0.1))) : g_r5_facmin;
      if (f > 1.0) f = 1.0;
      h *= f;
      rejected_last = 1;
      ++rej;
      if (!(h > 1e-13 * dt)) { status = 2; break; }
    }
  }
  if (W) free(W);
  if (nacc) *nacc = acc;
  if (nrej) *nrej = rej;
  if (status != 0)
    for (int i = 0; i < n; ++i) x[i] = NAN;
  return status;
}
/* ---------------------------------------------------------------------------------------------------------------
 * SEULEX-8: extrapolated linearly implicit Euler with a fixed column of eight (Deuflhard's SEULEX without order
 * selection) -- the integrator of the HEAVY envs of a PCG_INT_RODAS4 plan (cfg.coop_thr > 0), twin of seulex8_serial /
 * seulex8_lanes in pc-gym_amd/csrc/pcg_seulex.hpp.  The reference's CVODES integrates a stiff column at a cost that does
 * not depend on its batch-mates (integrator.py:163-182); on the GPU a launch is as long as its heaviest env, and this
 * scheme is parallel over j by construction (the kernels give row j of the tableau to lane j of eight):
 *   big step H from x:  for j = 0..7, n_j = j + 1:  theta_j = n_j (1 / H),  W_j = theta_j I - J(x)  (J frozen at x),
 *       y = x;  n_j times:  d = W_j^-1 f(y),  y = y + d                                  -> T_j
 *   Aitken-Neville in h:  for c = 1..7, rows j >= c (all rows of a column read the previous column):
 *       T_j <- fma(T_j - T_{j-1}, (n_j - c) / c, T_j)
 *   new state T_7 (order 8), error estimate T_7 - T_7' with T_7' the last row BEFORE the last column (order 7).
 *   Error norm: as rodas4 (mean square, end-point weights), tolerances SX_TOL x the plan's; accept iff E2 < 1;
 *   factor Q(SX_SAFETY E2^(-1/16)) in [SX_FACMIN, SX_FACMAX] (<= 1 after a rejection or a singular W_j).
 *   First step: min(dt, Q(SX_H0 h_r4)) with h_r4 the first step of rodas4.
 * ------------------------------------------------------------------------------------------------------------- */
static double g_sx_tol = 4.0, g_sx_h0 = 8.0, g_sx_safety = 0.8, g_sx_facmax = 4.0, g_sx_facmin = 0.1;
static int g_sx_ep = 1;
ORC_EXPORT void orc_set_seulex(double tol, double h0, double safety, double facmax, double facmin, int ep) {
  g_sx_tol = tol; g_sx_h0 = h0; g_sx_safety = safety; g_sx_facmax = facmax; g_sx_facmin = facmin; g_sx_ep = ep;
}
#define SX_K 8
static int seulex8(const orc_model* m, double* x, const double* u, double dt, double rtol, double atol, int max_steps,
                   double ep_frac, int ep_kmax, int32_t* nacc, int32_t* nrej) {
  const int n = m->nx;
  double T[SX_K][MAXNX], f[MAXNX], prev[MAXNX];
  me_ros_fac F;
  int acc = 0, rej = 0, status = 0;
  const double rt = g_sx_tol * rtol, at = g_sx_tol * atol;
  double H;
  {
    rhs_int(m, x, u, f);
    double d0 = rms_scaled(x, x, x, n, rtol, atol);
    double d1 = rms_scaled(f, x, x, n, rtol, atol);
    double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    H = fmin(qtrunc6(g_sx_h0 * (5.0 * h0)), dt);
  }
  const double ep_c = (ep_kmax > 0 && g_sx_ep) ? ep_frac * 1.4426950408889634 : 0.0;
  double t = 0.0;
  int rejected_last = 0;
  for (;;) {
    int last = 0;
    if (acc + rej >= max_steps) { status = 1; break; }
    if (t + H >= dt * (1.0 - 1e-14)) { H = dt - t; last = 1; }
    const double ih = 1.0 / H;
    int lu_ok = 1;
    for (int j = 0; j < SX_K; ++j) {
      const double theta = (double)(j + 1) * ih;
      me_ros_factor(m->p, u, x, theta, &F);
      lu_ok = lu_ok && F.ok;
      double* y = T[j];
      for (int i = 0; i < n; ++i) y[i] = x[i];
      for (int s = 0; s <= j; ++s) {
        rhs_int(m, y, u, f);
        me_ros_solve(&F, f);
        for (int i = 0; i < n; ++i) y[i] = y[i] + f[i];
      }
    }
    for (int c = 1; c < SX_K; ++c) {
      if (c == SX_K - 1)
        for (int i = 0; i < n; ++i) prev[i] = T[SX_K - 1][i];
      for (int j = SX_K - 1; j >= c; --j) {
        const double w = (double)(j + 1 - c) / (double)c;
        for (int i = 0; i < n; ++i) T[j][i] = fma(T[j][i] - T[j - 1][i], w, T[j][i]);
      }
    }
    const double* r = T[SX_K - 1];
    int kg[2];
    ep_exponents(m, u, ep_c, ep_c > 0.0 ? ep_kmax : 0, dt - (t + H), kg);
    const double sg[2] = {ldexp(1.0, -2 * kg[0]), ldexp(1.0, -2 * kg[1])};
    double E2 = 0.0;
    for (int i = 0; i < n; ++i) {
      double a0 = fabs(x[i]), a1 = fabs(r[i]);
      double q = (r[i] - prev[i]) / (at + rt * (a0 > a1 ? a0 : a1));
      E2 += (q * q) * sg[ep_group(m, i)];
    }
    E2 = E2 * (1.0 / n);
    if (!lu_ok) E2 = NAN;
    double fac = (E2 == E2) ? ((E2 == 0.0) ? g_sx_facmax : fmax(g_sx_facmin, qtrunc6(g_sx_safety * pow(E2, -1.0 / 16.0)))) : g_sx_facmin;
    if (E2 < 1.0) {
      fac = fmin(rejected_last ? 1.0 : g_sx_facmax, fac);
      t += H;
      H *= fac;
      for (int i = 0; i < n; ++i) x[i] = r[i];
      rejected_last = 0;
      ++acc;
      if (last) break;
    } else {
      fac = fmin(1.0, fac);
      H *= fac;
      rejected_last = 1;
      ++rej;
      if (!(H > 1e-13 * dt)) { status = 2; break; }
    }
  }
  if (nacc) *nacc = acc;
  if (nrej) *nrej = rej;
  if (status != 0)
    for (int i = 0; i < n; ++i) x[i] = NAN;
  return status;
}
/* The cooperative rule of PCG_INT_RODAS4 plans (twin of MEImpl::coop_key, pcg_models.hpp): predicted attempts of the pair
 * for this env step, in exact arithmetic -- piecewise-linear log2 by exponent extraction, IEEE operations. */
static double plog2(double v) {
  int e;
  const double m = frexp(v, &e); /* [0.5, 1) */
  return (double)(e - 1) + (2.0 * m - 1.0);
}
static int me_coop_model(const orc_model* m) { return m->model_id == PCG_MODEL_ME && m->p[4] == 2.0 && g_ros4_structured; }
static double me_coop_key(const orc_model* m, const double* u, double d1) {
  const double iVl = 1 / m->p[0], iVg = 1 / m->p[1];
  const double a = u[0] * iVl, c = u[1] * iVg;
  const double mn = fmin(a, c);
  return ((-30.0 - 10.0 * plog2(mn)) + 3.6 / mn) + 4.0 * plog2(fmax(d1, 1.0));
}
/* the Rosenbrock plan on one env: SEULEX-8 where the rule picks the env, the pair elsewhere (twin of seulex8_if_heavy) */
static int rodas4_plan(int integ, const orc_model* m, double* x, const double* u, double dt, double rtol, double atol, int max_steps,
                       double ep_frac, int ep_kmax, double coop_thr, int32_t* nacc, int32_t* nrej) {
  if (coop_thr > 0.0 && me_coop_model(m)) {
    double f0[MAXNX];
    rhs_int(m, x, u, f0);
    const double d1 = rms_scaled(f0, x, x, m->nx, rtol, atol);
    if (me_coop_key(m, u, d1) >= coop_thr) return seulex8(m, x, u, dt, rtol, atol, max_steps, ep_frac, ep_kmax, nacc, nrej);
  }
  if (integ == PCG_INT_RODAS5) return rodas5(m, x, u, dt, rtol, atol, max_steps, ep_frac, ep_kmax, nacc, nrej);
  return rodas4(m, x, u, dt, rtol, atol, max_steps, ep_frac, ep_kmax, nacc, nrej);
}
/* test hook: the rule's key for every env of a batch (x [nx][B], u [nu][B]) */
ORC_EXPORT int orc_coop_key(const pcg_env_cfg* c, int64_t B, const double* x, const double* u, double* key) {
  int nx = c->nx, nu = c->na + c->ndm;
  orc_model m = {c->model_id, nx, nu, c->params};
  if (!me_coop_model(&m)) return PCG_E_UNSUPPORTED;
  for (int64_t b = 0; b < B; ++b) {
    double xi[MAXNX], ui[PCG_MAX_NU], f0[MAXNX];
    for (int i = 0; i < nx; ++i) xi[i] = x[(size_t)i * B + b];
    for (int i = 0; i < nu; ++i) ui[i] = u[(size_t)i * B + b];
    rhs_int(&m, xi, ui, f0);
    key[b] = me_coop_key(&m, ui, rms_scaled(f0, xi, xi, nx, c->rtol, c->atol));
  }
  return 0;
}

/* calibration / test hook: SEULEX-8 for EVERY env of the batch (the plan's rule picks the heavy ones: coop_heavy()) */
ORC_EXPORT int orc_seulex8(const pcg_env_cfg* c, int64_t B, double* x, const double* u, int32_t* nsteps) {
  int nx = c->nx, nu = c->na + c->ndm;
  if (c->model_id != PCG_MODEL_ME) return PCG_E_UNSUPPORTED;
  orc_model m = {c->model_id, nx, nu, c->params};
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t b = 0; b < B; ++b) {
    double xi[MAXNX], ui[PCG_MAX_NU];
    int32_t na_ = 0, nr_ = 0;
    for (int i = 0; i < nx; ++i) xi[i] = x[(size_t)i * B + b];
    for (int i = 0; i < nu; ++i) ui[i] = u[(size_t)i * B + b];
    seulex8(&m, xi, ui, c->dt, c->rtol, c->atol, c->max_steps, c->ep_frac, c->ep_kmax, &na_, &nr_);
    for (int i = 0; i < nx; ++i) x[(size_t)i * B + b] = xi[i];
    if (nsteps) { nsteps[b] = na_; nsteps[B + b] = nr_; }
  }
  return 0;
}

/* ------------------------------------------------------------------------- */
/* Counter-based RNG: Philox4x32-10 (Salmon et al., SC'11; Random123 v1.09)   */
/* ------------------------------------------------------------------------- */
ORC_EXPORT void orc_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    uint32_t n1 = (uint32_t)p1;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

/* RNG contract shared with the kernels (DESIGN.md "RNG"):
 *   key = (seed_lo, seed_hi); ctr = (env_lo, env_hi, t, purpose + pair_index)
 *   purpose: 0x100 obs noise, 0x200 Gaussian disturbance, 0x300 reset uncertainty
 *   uniforms: one block -> two 53-bit uniforms;  normals (v2): one block -> two fp32 Box-Muller pairs */
#define ORC_RNG_NOISE 0x100u
#define ORC_RNG_DIST 0x200u
#define ORC_RNG_RESET 0x300u

static void rng_uniform2(uint64_t seed, uint64_t env, uint32_t t, uint32_t stream, double* u0, double* u1) {
  uint32_t ctr[4] = {(uint32_t)env, (uint32_t)(env >> 32), t, stream};
  uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t o[4];
  orc_philox4x32_10(ctr, key, o);
  *u0 = (double)(((uint64_t)(o[0] >> 5) << 26) | (uint64_t)(o[1] >> 6)) * (1.0 / 9007199254740992.0);
  *u1 = (double)(((uint64_t)(o[2] >> 5) << 26) | (uint64_t)(o[3] >> 6)) * (1.0 / 9007199254740992.0);
}

/* Box-Muller in fp32: the exact IEEE-754 single-precision operation sequence of box_muller_f32 in
 * pc-gym_amd/csrc/pcg_kernels.hpp (DESIGN.md "RNG", contract v2) -- fmaf where the kernel has fmaf, no contraction
 * elsewhere (-ffp-contract=off), correctly rounded divide / sqrtf / rintf: bit-identical variates on both sides. */
static void box_muller_f32(uint32_t w0, uint32_t w1, float* z0, float* z1) {
  const float u0 = (float)(((w0 >> 9) << 1) | 1u) * 0x1p-24f;
  const float u1 = (float)(w1 >> 8) * 0x1p-24f;
  int e;
  float m = frexpf(u0, &e); /* [0.5, 1) */
  if (m < 0.70710678f) { m = m + m; e = e - 1; }
  const float s = (m - 1.0f) / (m + 1.0f);
  const float q = s * s;
  float p = 0.22222222f;
  p = fmaf(p, q, 0.28571429f);
  p = fmaf(p, q, 0.4f);
  p = fmaf(p, q, 0.66666667f);
  const float lm = fmaf(s * q, p, s + s);
  const float fe = (float)e;
  const float ln = fmaf(fe, 0.693359375f, fmaf(fe, -2.12194440e-4f, lm));
  float arg = -2.0f * ln;
  if (!(arg > 0.0f)) arg = 0.0f;
  const float r = sqrtf(arg);
  const float x = u1 + u1;
  const float n = rintf(x + x);
  const float a = fmaf(n, -0.5f, x) * 3.14159274f;
  const float a2 = a * a;
  float ps = 2.7557319e-6f;
  ps = fmaf(ps, a2, -1.9841270e-4f);
  ps = fmaf(ps, a2, 8.3333333e-3f);
  ps = fmaf(ps, a2, -0.16666667f);
  const float sy = fmaf(a * a2, ps, a);
  float pc = 2.4801587e-5f;
  pc = fmaf(pc, a2, -1.3888889e-3f);
  pc = fmaf(pc, a2, 4.1666667e-2f);
  pc = fmaf(pc, a2, -0.5f);
  const float cy = fmaf(a2, pc, 1.0f);
  const int qd = (int)n & 3;
  const float ss = (qd & 1) ? cy : sy, cc = (qd & 1) ? sy : cy;
  *z1 = r * ((qd & 2) ? -ss : ss);
  *z0 = r * (((qd + 1) & 2) ? -cc : cc);
}

/* variate idx of a purpose: pair idx/2 lives in Philox block (purpose + idx/4), words (0,1) / (2,3) */
static double rng_normal(uint64_t seed, uint64_t env, uint32_t t, uint32_t purpose, int idx) {
  uint32_t pair = (uint32_t)(idx >> 1);
  uint32_t ctr[4] = {(uint32_t)env, (uint32_t)(env >> 32), t, purpose + (pair >> 1)};
  uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t o[4];
  orc_philox4x32_10(ctr, key, o);
  float z0, z1;
  box_muller_f32((pair & 1u) ? o[2] : o[0], (pair & 1u) ? o[3] : o[1], &z0, &z1);
  return (double)((idx & 1) ? z1 : z0);
}

static double rng_uniform(uint64_t seed, uint64_t env, uint32_t t, uint32_t purpose, int idx) {
  double u0, u1;
  rng_uniform2(seed, env, t, purpose + (uint32_t)(idx >> 1), &u0, &u1);
  return (idx & 1) ? u1 : u0;
}

ORC_EXPORT double orc_rng_normal(uint64_t seed, uint64_t env, uint32_t t, uint32_t purpose, int idx) {
  return rng_normal(seed, env, t, purpose, idx);
}
ORC_EXPORT double orc_rng_uniform(uint64_t seed, uint64_t env, uint32_t t, uint32_t purpose, int idx) {
  return rng_uniform(seed, env, t, purpose, idx);
}
/* box_muller_f32 on n word pairs (tests/test_rng_accuracy.py: the polynomials against a long double Box-Muller) */
ORC_EXPORT void orc_box_muller_f32_n(const uint32_t* w0, const uint32_t* w1, int64_t n, float* z0, float* z1) {
  for (int64_t i = 0; i < n; ++i) box_muller_f32(w0[i], w1[i], &z0[i], &z1[i]);
}

/* ------------------------------------------------------------------------- */
/* make_env.step for ONE environment, pcgym.py:350-500, statement by statement */
/* ------------------------------------------------------------------------- */
typedef struct {
  double* state;   /* [Nobs]  reference self.state = [x | SP | d]  in/out */
  double* a_save;  /* [na]    in/out (a_delta) */
  int32_t t;       /* in/out */
  double* u_prev;  /* [na]    in/out (custom_reward family: self.u_prev; NaN = attribute not set yet) */
} orc_env;

static int cfg_nobs(const pcg_env_cfg* c) { return c->nx + c->nsp_obs + c->nd + c->nunc; }
static int cfg_nu(const pcg_env_cfg* c) { return c->na + c->ndm; }

/* constraint_check + con_checker, pcgym.py:580-615, 560-577.
 * The user callable g(x,u) is represented by its affine rows (con_A, con_b). */
static int constraint_check(const pcg_env_cfg* c, const double* state, const double* uk, double* g_out) {
  int nobs = cfg_nobs(c), nu = cfg_nu(c);
  double s[PCG_MAX_NOBS], in[PCG_MAX_NU];
  for (int i = 0; i < nobs; ++i) s[i] = state[i];
  for (int i = 0; i < nu; ++i) in[i] = uk[i];
  if (c->flags & PCG_F_REF_COMPAT) {
    /* Q3: the reference "de-normalises" the physical input/state again (pcgym.py:597-608).
     * numpy broadcasting of a_space (na) against uk (Nu) is only defined for Nu==na or na==1. */
    if (c->flags & PCG_F_NORMALISE_A)
      for (int i = 0; i < nu; ++i) {
        int j = (c->na == 1) ? 0 : i;
        in[i] = (in[i] + 1) * (c->a_high[j] - c->a_low[j]) / 2 + c->a_low[j];
      }
    if (c->flags & PCG_F_NORMALISE_O)
      for (int i = 0; i < nobs; ++i) s[i] = (s[i] + 1) * (c->o_high[i] - c->o_low[i]) / 2 + c->o_low[i];
  }
  int violated = 0;
  for (int r = 0; r < c->ncon; ++r) {
    const double* row = c->con_A + (size_t)r * (nobs + nu);
    double g = 0.0;
    for (int i = 0; i < nobs; ++i) g += row[i] * s[i];
    for (int i = 0; i < nu; ++i) g += row[nobs + i] * in[i];
    g -= c->con_b[r];
    if (g_out) g_out[r] = g;
    if (g > 0) violated = 1;
  }
  return violated;
}

typedef struct {
  double* obs;    /* [Nobs] */
  double rew;
  uint8_t done, viol;
  double* g;      /* [ncon] or NULL */
  double* g_pre;  /* [ncon] or NULL */
  int32_t nacc, nrej;
  uint8_t status; /* PCG_ST_* */
  double uk[PCG_MAX_NU];
} orc_out;

static void env_step(const pcg_env_cfg* c, orc_env* e, const double* action_in, const double* d_env,
                     uint64_t seed, uint64_t env_id, orc_out* o, const double* params) {
  int nx = c->nx, na = c->na, nsp = c->nsp, nd = c->nd, ndm = c->ndm;
  int nobs = cfg_nobs(c), nu = cfg_nu(c);
  double action[PCG_MAX_NA];
  double* uk = o->uk;
  int t = e->t;
  int tn = (t + 1 < c->N) ? t + 1 : c->N - 1; /* schedule index clamp (reference would IndexError) */
  int tc = (t < c->N) ? t : c->N - 1;
  for (int i = 0; i < nu; ++i) uk[i] = 0.0; /* :371 */
  for (int i = 0; i < na; ++i) action[i] = action_in[i];
  if (c->flags & PCG_F_NORMALISE_A) /* :372-375 */
    for (int i = 0; i < na; ++i) action[i] = (action[i] + 1) * (c->a_high[i] - c->a_low[i]) / 2 + c->a_low[i];
  if ((c->flags & PCG_F_NORMALISE_A) && (c->flags & PCG_F_A_DELTA)) { /* :376-383 */
    if (c->flags & PCG_F_REF_COMPAT) /* Q1: de-normalised a second time */
      for (int i = 0; i < na; ++i) action[i] = (action[i] + 1) * (c->a_high[i] - c->a_low[i]) / 2 + c->a_low[i];
    for (int i = 0; i < na; ++i) {
      action[i] = e->a_save[i] + action[i]; /* Q2: the unclipped sum drives the plant */
      double s = action[i];
      if (s < c->a_act_low[i]) s = c->a_act_low[i];
      if (s > c->a_act_high[i]) s = c->a_act_high[i];
      e->a_save[i] = s;
    }
  }
  /* disturbances :386-412 */
  for (int i = 0; i < na; ++i) uk[i] = action[i];
  if (ndm > 0) {
    for (int j = 0; j < ndm; ++j) /* :400-404 -- the env's own parameter value when parameters are uncertain (Q11) */
      uk[na + j] = (c->nunc > 0 && c->d_param_index) ? params[c->d_param_index[j]] : c->d_default[j];
    for (int k = 0; k < nd; ++k) {
      double v;
      if (d_env) v = d_env[k];
      else v = c->d_sched[(size_t)k * c->N + tn]; /* :394  index t+1 (Q6) */
      if (c->flags & PCG_F_GAUSS_DIST) {
        v += c->d_sigma[k] * rng_normal(seed, env_id, (uint32_t)t, ORC_RNG_DIST, k);
        if (v < c->d_clip_lo[k]) v = c->d_clip_lo[k];
        if (v > c->d_clip_hi[k]) v = c->d_clip_hi[k];
      }
      uk[na + c->d_slot[k]] = v;
      e->state[nx + c->nsp_obs + k] = v; /* :409-410 */
    }
  }
  o->viol = 0;
  uint8_t done = 0;
  if (t == 0 && c->ncon > 0) { /* :414-420 pre-step check */
    double gp[PCG_MAX_NCON];
    int v = constraint_check(c, e->state, uk, gp);
    if (o->g_pre) memcpy(o->g_pre, gp, sizeof(double) * c->ncon);
    if (v && (c->flags & PCG_F_DONE_ON_CONS)) done = 1;
  }
  /* integrate :423-429 */
  orc_model m = {c->model_id, nx, nu, params}; /* per-env parameters when uncertain (pcgym.py:301-310) */
  o->nacc = o->nrej = 0;
  int ist = 0;
  if (c->integrator_id == PCG_INT_RK4) rk4(&m, e->state, uk, c->dt, c->substeps);
  else if (c->integrator_id == PCG_INT_RODAS3)
    ist = rodas3(&m, e->state, uk, c->dt, c->rtol, c->atol, c->max_steps, &o->nacc, &o->nrej);
  else if (c->integrator_id == PCG_INT_RK4G)
    ist = rk4g(&m, e->state, uk, c->dt, c->substeps, c->rtol, c->atol, c->max_steps, &o->nacc, &o->nrej);
  else if (c->integrator_id == PCG_INT_T5G)
    ist = t5g(&m, e->state, uk, c->dt, c->substeps, c->rtol, c->atol, c->max_steps, &o->nacc, &o->nrej);
  else if (c->integrator_id == PCG_INT_CV8) cv8(&m, e->state, uk, c->dt, c->substeps);
  else if (c->integrator_id == PCG_INT_TSIT5)
    ist = tsit5(&m, e->state, uk, c->dt, c->rtol, c->atol, c->max_steps, &o->nacc, &o->nrej);
  else if (c->integrator_id == PCG_INT_RODAS4 || c->integrator_id == PCG_INT_RODAS5)
    ist = rodas4_plan(c->integrator_id, &m, e->state, uk, c->dt, c->rtol, c->atol, c->max_steps, c->ep_frac, c->ep_kmax, c->coop_thr, &o->nacc, &o->nrej);
  else ist = dopri5(&m, e->state, uk, c->dt, c->rtol, c->atol, c->max_steps, &o->nacc, &o->nrej);
  if (ist == 0)
    for (int i = 0; i < nx; ++i)
      if (!isfinite(e->state[i])) ist = PCG_ST_NONFINITE;
  o->status = (uint8_t)ist;
  /* SP slot :432-438 uses SP[k][t] with the OLD t (Q5) */
  for (int k = 0; k < c->nsp_obs; ++k) e->state[nx + k] = c->sp[(size_t)k * c->N + tc];
  e->t = t + 1; /* :441 */
  int violated = 0;
  if (c->ncon > 0) { /* :443-446 */
    violated = constraint_check(c, e->state, uk, o->g);
    if (violated && (c->flags & PCG_F_DONE_ON_CONS)) done = 1;
  }
  o->viol = (uint8_t)violated;
  if (e->t == c->N - 1) done = 1; /* :448-449 */
  o->done = done;
  /* obs + noise :452-466 */
  for (int i = 0; i < nobs; ++i) o->obs[i] = e->state[i];
  if (c->flags & PCG_F_NOISE)
    for (int i = 0; i < nx; ++i)
      o->obs[i] += rng_normal(seed, env_id, (uint32_t)t, ORC_RNG_NOISE, i) * e->state[i] * c->noise_pct[i];
  /* reward :470-482 */
  double r = 0.0;
  if (c->flags & PCG_F_REWARD_BATCH) { /* :502-532 */
    if (e->t == c->N - 1) {
      for (int k = 0; k < c->nrew; ++k) {
        if (c->flags & PCG_F_MAXIMISE) r += e->state[c->rew_index[k]] * c->r_scale[k];
        else r -= e->state[c->rew_index[k]] * c->r_scale[k];
      }
      if ((c->flags & PCG_F_R_PENALTY) && violated) r -= 1000;
    }
  } else { /* :535-558 */
    int ti = (e->t < c->N) ? e->t : c->N - 1;
    for (int k = 0; k < nsp; ++k) {
      double d = e->state[c->sp_index[k]] - c->sp[(size_t)k * c->N + ti];
      r += (-(d * d)) * c->r_scale[k];
      if ((c->flags & PCG_F_R_PENALTY) && violated) r -= 1000; /* Q4: once per SP key */
    }
  }
  if (c->flags & PCG_F_REWARD_TRACK) {
    /* the custom_reward family of the paper scripts, called as custom_reward_f(self, self.obs, uk, violated)
     * (pcgym.py:470-471).  pc-gym_paper/train_policies/cstr/custom_reward.py:3-39 line by line; the R_u term is
     * Biofilm/biofilm_train.py:36-39, the box term constraint_showcase/custom_reward.py:40-62. */
    double cost = 0.0;
    int ti = (e->t < c->N) ? e->t : c->N - 1;
    for (int k = 0; k < nsp; ++k) { /* :10-24 */
      int i = c->sp_index[k];
      double lo = c->o_low[i], hi = c->o_high[i];
      double xv = o->obs[i];
      if ((c->flags & PCG_F_REWARD_CRYST) && i == 5) /* crystalisation/cryst_train.py:24 */
        xv = pow(o->obs[2] * o->obs[0] / (o->obs[1] * o->obs[1]) - 1, 0.5);
      if ((c->flags & PCG_F_REWARD_CRYST) && i == 6) /* :25 */
        xv = o->obs[1] / o->obs[0];
      double x_normalized = (xv - lo) / (hi - lo);
      double setpoint_normalized = (c->sp[(size_t)k * c->N + ti] - lo) / (hi - lo);
      cost += ((x_normalized - setpoint_normalized) * (x_normalized - setpoint_normalized)) * c->r_scale[k];
    }
    for (int j = 0; j < c->na; ++j) { /* :25-34 */
      double up = e->u_prev[j];
      if (up != up) up = uk[j]; /* :7-8 first call: self.u_prev = u */
      double u_normalized = (uk[j] - c->a_low[j]) / (c->a_high[j] - c->a_low[j]);
      double u_prev_norm = (up - c->a_low[j]) / (c->a_high[j] - c->a_low[j]);
      e->u_prev[j] = uk[j];
      cost += c->rew_R_du * ((u_normalized - u_prev_norm) * (u_normalized - u_prev_norm));
      cost += c->rew_R_u * (u_normalized * u_normalized);
    }
    if (violated) /* constraint_showcase/custom_reward.py:40-62 */
      for (int q = 0; q < c->rew_nbox; ++q) {
        int i = c->rew_box_index[q];
        double lo = c->o_low[i], hi = c->o_high[i];
        double x_normalized = (o->obs[i] - lo) / (hi - lo);
        double lower_normalized = (c->rew_box_lo[q] - lo) / (hi - lo);
        double upper_normalized = (c->rew_box_hi[q] - lo) / (hi - lo);
        if (x_normalized > upper_normalized) cost += (x_normalized - upper_normalized) * (x_normalized - upper_normalized);
        else if (x_normalized < lower_normalized) cost += (lower_normalized - x_normalized) * (lower_normalized - x_normalized);
      }
    r = -cost;
  }
  o->rew = r;
  /* normalise :483-489 */
  if (c->flags & PCG_F_NORMALISE_O)
    for (int i = 0; i < nobs; ++i) o->obs[i] = 2 * (o->obs[i] - c->o_low[i]) / (c->o_high[i] - c->o_low[i]) - 1;
  /* partial observation :495-498 */
  if (c->obs_mask)
    for (int i = 0; i < nx; ++i)
      if (!c->obs_mask[i]) o->obs[i] = 0;
}

/* make_env.reset for one env, pcgym.py:263-349 */
static void env_reset(const pcg_env_cfg* c, orc_env* e, uint64_t seed, uint64_t env_id, double* obs) {
  int nx = c->nx, nsp = c->nsp_obs, nd = c->nd, nobs = cfg_nobs(c);
  e->t = 0; /* :279 */
  for (int i = 0; i < nx + nsp; ++i) e->state[i] = c->x0[i]; /* :284 */
  if (c->x0_unc) /* :285-288, apply_uncertainties :255-261 */
    for (int i = 0; i < nx; ++i) {
      double pct = c->x0_unc[i];
      if (pct == 0.0) continue;
      if (c->flags & PCG_F_X0_NORMAL)
        e->state[i] = c->x0[i] + pct * c->x0[i] * rng_normal(seed, env_id, 0u, ORC_RNG_RESET, i);
      else
        e->state[i] = c->x0[i] * (1 + pct * (2.0 * rng_uniform(seed, env_id, 0u, ORC_RNG_RESET, i) - 1.0));
    }
  for (int k = 0; k < nd; ++k) e->state[nx + nsp + k] = c->d_sched[(size_t)k * c->N + 0]; /* :291-298 (Q6: index 0) */
  for (int j = 0; j < c->nunc; ++j) { /* :301-310, apply_uncertainties :255-261 */
    /* (an index past the parameters = an inert entry: empirical_distribution['x0'], sampled and observed only) */
    double orig = c->unc_index[j] < c->n_params ? c->params[c->unc_index[j]] : 0.0, pct = c->unc_pct[j], v;
    int ri = nx + j;
    if (c->flags & PCG_F_UNC_EMPIRICAL) { /* :311-316 np.random.choice(samples): uniform index */
      int len = c->unc_emp_off[j + 1] - c->unc_emp_off[j];
      int idx = (int)(rng_uniform(seed, env_id, 0u, ORC_RNG_RESET, ri) * (double)len);
      if (idx > len - 1) idx = len - 1;
      v = c->unc_emp[c->unc_emp_off[j] + idx];
    } else if (c->flags & PCG_F_X0_NORMAL) v = orig + pct * orig * rng_normal(seed, env_id, 0u, ORC_RNG_RESET, ri);
    else v = orig * (1 + pct * (2.0 * rng_uniform(seed, env_id, 0u, ORC_RNG_RESET, ri) - 1.0));
    e->state[nx + nsp + nd + j] = v;
  }
  if (c->flags & PCG_F_A_DELTA) /* :319-320 */
    for (int i = 0; i < c->na; ++i) e->a_save[i] = c->a_0[i];
  for (int i = 0; i < nobs; ++i) obs[i] = e->state[i];
  if (c->flags & PCG_F_NORMALISE_O) /* :331-337 */
    for (int i = 0; i < nobs; ++i) obs[i] = 2 * (obs[i] - c->o_low[i]) / (c->o_high[i] - c->o_low[i]) - 1;
  if (c->obs_mask) /* :344-347 */
    for (int i = 0; i < nx; ++i)
      if (!c->obs_mask[i]) obs[i] = 0;
}

/* ------------------------------------------------------------------------- */
/* Batched entry points over the SAME SoA buffers the HIP library takes        */
/* (host memory).  The SP / disturbance slots of the reference state vector    */
/* are carried in io->obs-shaped scratch `state_slots` [nsp+nd][B].            */
/* ------------------------------------------------------------------------- */
ORC_EXPORT int orc_rhs(int model_id, const double* params, int nx, int nu, int64_t B, const double* x,
                       const double* u, double* dx) {
  orc_model m = {model_id, nx, nu, params};
  for (int64_t b = 0; b < B; ++b) {
    double xi[MAXNX], ui[PCG_MAX_NU], di[MAXNX];
    for (int i = 0; i < nx; ++i) xi[i] = x[(size_t)i * B + b];
    for (int i = 0; i < nu; ++i) ui[i] = u[(size_t)i * B + b];
    rhs(&m, xi, ui, di);
    for (int i = 0; i < nx; ++i) dx[(size_t)i * B + b] = di[i];
  }
  return 0;
}

ORC_EXPORT int orc_integrate(const pcg_env_cfg* c, int64_t B, double* x, const double* u, int32_t* nsteps) {
  int nx = c->nx, nu = cfg_nu(c);
  orc_model m = {c->model_id, nx, nu, c->params};
  for (int64_t b = 0; b < B; ++b) {
    double xi[MAXNX], ui[PCG_MAX_NU];
    int32_t na_ = 0, nr_ = 0;
    for (int i = 0; i < nx; ++i) xi[i] = x[(size_t)i * B + b];
    for (int i = 0; i < nu; ++i) ui[i] = u[(size_t)i * B + b];
    if (c->integrator_id == PCG_INT_RK4) rk4(&m, xi, ui, c->dt, c->substeps);
    else if (c->integrator_id == PCG_INT_RODAS3) rodas3(&m, xi, ui, c->dt, c->rtol, c->atol, c->max_steps, &na_, &nr_);
    else if (c->integrator_id == PCG_INT_RK4G) rk4g(&m, xi, ui, c->dt, c->substeps, c->rtol, c->atol, c->max_steps, &na_, &nr_);
    else if (c->integrator_id == PCG_INT_T5G) t5g(&m, xi, ui, c->dt, c->substeps, c->rtol, c->atol, c->max_steps, &na_, &nr_);
    else if (c->integrator_id == PCG_INT_CV8) cv8(&m, xi, ui, c->dt, c->substeps);
    else if (c->integrator_id == PCG_INT_TSIT5) tsit5(&m, xi, ui, c->dt, c->rtol, c->atol, c->max_steps, &na_, &nr_);
    else if (c->integrator_id == PCG_INT_RODAS4 || c->integrator_id == PCG_INT_RODAS5)
      rodas4_plan(c->integrator_id, &m, xi, ui, c->dt, c->rtol, c->atol, c->max_steps, c->ep_frac, c->ep_kmax, c->coop_thr, &na_, &nr_);
    else dopri5(&m, xi, ui, c->dt, c->rtol, c->atol, c->max_steps, &na_, &nr_);
    for (int i = 0; i < nx; ++i) x[(size_t)i * B + b] = xi[i];
    if (nsteps) { nsteps[b] = na_; nsteps[B + b] = nr_; }
  }
  return 0;
}

/* slots: [nsp+nd][B] host scratch holding the SP / disturbance slots of the reference's
 * state vector between calls (written by orc_reset / orc_step). */
ORC_EXPORT int orc_step(const pcg_env_cfg* c, const pcg_buffers* io, double* slots, int32_t t_scalar,
                        uint64_t seed, int64_t env_offset, int n_threads) {
  if ((c->flags & PCG_F_REWARD_TRACK) && !io->u_prev) return PCG_E_NULL;
  int nx = c->nx, na = c->na, nsp = c->nsp_obs, nd = c->nd, nobs = cfg_nobs(c), ncon = c->ncon;
  int64_t B = io->B;
  (void)n_threads;
#ifdef _OPENMP
#pragma omp parallel for schedule(static) num_threads(n_threads > 0 ? n_threads : 1)
#endif
  for (int64_t b = 0; b < B; ++b) {
    double state[PCG_MAX_NOBS], asave[PCG_MAX_NA], act[PCG_MAX_NA], denv[PCG_MAX_NDM];
    double obs[PCG_MAX_NOBS], g[PCG_MAX_NCON], gp[PCG_MAX_NCON];
    for (int i = 0; i < nx; ++i) state[i] = io->x[(size_t)i * B + b];
    for (int i = 0; i < nsp + nd + c->nunc; ++i) state[nx + i] = slots ? slots[(size_t)i * B + b] : 0.0;
    double params[PCG_MAX_PARAMS];
    for (int i = 0; i < c->n_params; ++i) params[i] = c->params[i];
    for (int j = 0; j < c->nunc; ++j) {
      double v = io->p_unc[(size_t)j * B + b];
      if (c->unc_index[j] < c->n_params) params[c->unc_index[j]] = v;
      state[nx + nsp + nd + j] = v;
    }
    for (int i = 0; i < na; ++i) act[i] = io->a[(size_t)i * B + b];
    if (io->a_save)
      for (int i = 0; i < na; ++i) asave[i] = io->a_save[(size_t)i * B + b];
    if (io->d)
      for (int i = 0; i < nd; ++i) denv[i] = io->d[(size_t)i * B + b];
    double uprev[PCG_MAX_NA];
    if (io->u_prev)
      for (int i = 0; i < na; ++i) uprev[i] = io->u_prev[(size_t)i * B + b];
    orc_env e = {state, asave, io->t ? io->t[b] : t_scalar, uprev};
    orc_out o;
    o.obs = obs;
    o.g = g;
    o.g_pre = gp;
    int t_old = e.t;
    env_step(c, &e, act, io->d ? denv : NULL, seed, (uint64_t)(env_offset + b), &o, params);
    for (int i = 0; i < nx; ++i) io->x[(size_t)i * B + b] = state[i];
    if (slots)
      for (int i = 0; i < nsp + nd + c->nunc; ++i) slots[(size_t)i * B + b] = state[nx + i];
    if (io->a_save)
      for (int i = 0; i < na; ++i) io->a_save[(size_t)i * B + b] = asave[i];
    if (io->u_prev)
      for (int i = 0; i < na; ++i) io->u_prev[(size_t)i * B + b] = uprev[i];
    if (io->t) io->t[b] = e.t;
    for (int i = 0; i < nobs; ++i) io->obs[(size_t)i * B + b] = obs[i];
    io->rew[b] = o.rew;
    io->done[b] = o.done;
    if (io->viol) io->viol[b] = o.viol;
    if (io->status && o.status) io->status[b] = o.status; /* sticky, like the kernels: only failures are written */
    if (io->g)
      for (int i = 0; i < ncon; ++i) io->g[(size_t)i * B + b] = g[i];
    if (io->g_pre && t_old == 0)
      for (int i = 0; i < ncon; ++i) io->g_pre[(size_t)i * B + b] = gp[i];
    if (io->nsteps) { io->nsteps[b] = o.nacc; io->nsteps[B + b] = o.nrej; }
  }
  return 0;
}

/* The timed CPU baseline (bench.py: cpu_baseline) on a many-core host: (1) orc_reset writes every SoA buffer first, so it
 * runs on the SAME static partition of the envs as orc_step -- each thread's slice of every row is first touched, hence
 * placed, on that thread's NUMA node; (2) the team is pinned, thread i on the (i n_cpu / n)-th CPU of the process's mask
 * (spread over the sockets; OMP_PROC_BIND cannot be relied on: another OpenMP runtime is already initialised in the process);
 * orc_unpin_threads() gives every pinned worker (and the calling thread) the process's mask back. */
static int g_reset_threads = 1;
ORC_EXPORT void orc_set_reset_threads(int n) { g_reset_threads = n > 0 ? n : 1; }
static cpu_set_t g_mask0;
static int g_mask0_valid = 0;
static int g_pinned_team = 0; /* the largest team orc_pin_threads has pinned */
ORC_EXPORT int orc_pin_threads(int n) {
  if (n < 1) return -1;
  if (!g_mask0_valid) {
    if (sched_getaffinity(0, sizeof g_mask0, &g_mask0) != 0) return -2;
    g_mask0_valid = 1;
  }
  int cpus[CPU_SETSIZE], nc = 0;
  for (int i = 0; i < CPU_SETSIZE; ++i)
    if (CPU_ISSET(i, &g_mask0)) cpus[nc++] = i;
  if (nc == 0) return -3;
  int bad = 0;
  (void)cpus;
  if (n > g_pinned_team) g_pinned_team = n;
#ifdef _OPENMP
#pragma omp parallel num_threads(n) reduction(+ : bad)
  {
    const int i = omp_get_thread_num();
    cpu_set_t m;
    CPU_ZERO(&m);
    CPU_SET(cpus[(int)(((int64_t)i * nc) / n) % nc], &m);
    if (sched_setaffinity(0, sizeof m, &m) != 0) ++bad;
  }
#endif
  return bad;
}
/* every worker of the largest team pinned so far gets the process's mask back, not only the calling thread: a later,
 * smaller team must not inherit the stale pinning of a larger one (the OpenMP runtime keeps its workers) */
ORC_EXPORT int orc_unpin_threads(void) {
  if (!g_mask0_valid) return 0;
  int bad = 0;
#ifdef _OPENMP
  const int n = g_pinned_team > 0 ? g_pinned_team : 1;
#pragma omp parallel num_threads(n) reduction(+ : bad)
  {
    if (sched_setaffinity(0, sizeof g_mask0, &g_mask0) != 0) ++bad;
  }
#endif
  if (sched_setaffinity(0, sizeof g_mask0, &g_mask0) != 0) ++bad;
  return bad;
}

ORC_EXPORT int orc_reset(const pcg_env_cfg* c, const pcg_buffers* io, double* slots, const uint8_t* mask,
                         uint64_t seed, int64_t env_offset) {
  int nx = c->nx, na = c->na, nsp = c->nsp_obs, nd = c->nd, nobs = cfg_nobs(c);
  int64_t B = io->B;
#ifdef _OPENMP
#pragma omp parallel for schedule(static) num_threads(g_reset_threads)
#endif
  for (int64_t b = 0; b < B; ++b) {
    if (mask && !mask[b]) continue;
    double state[PCG_MAX_NOBS], asave[PCG_MAX_NA], obs[PCG_MAX_NOBS];
    orc_env e = {state, asave, 0, NULL};
    env_reset(c, &e, seed, (uint64_t)(env_offset + b), obs);
    for (int i = 0; i < nx; ++i) io->x[(size_t)i * B + b] = state[i];
    if (slots)
      for (int i = 0; i < nsp + nd + c->nunc; ++i) slots[(size_t)i * B + b] = state[nx + i];
    for (int j = 0; j < c->nunc; ++j) io->p_unc[(size_t)j * B + b] = state[nx + nsp + nd + j];
    if (io->a_save && (c->flags & PCG_F_A_DELTA))
      for (int i = 0; i < na; ++i) io->a_save[(size_t)i * B + b] = asave[i];
    if (io->t) io->t[b] = 0;
    for (int i = 0; i < nobs; ++i) io->obs[(size_t)i * B + b] = obs[i];
  }
  return 0;
}

ORC_EXPORT int orc_version(void) { return PCG_ABI_VERSION; }
