// One restart of newton! on the host (csrc/host_numerics.cpp: newton_restart_poly, newton_restart_next) on named inputs: the
// coefficients P of Psi, R of the next start vector and its norm beta that the two functions must return, bit for bit.
// Included by tests/sanitize_host_numerics.cpp.
//
// How the expected values were produced: NOT by the functions under test.  The lines of qp_newton_step that did this algebra in the
// commit before it moved into host_numerics.cpp (engine_krylov.hip, from `const int mp = m + 1;` to the end of the conversion to the
// stored basis by nu) were copied verbatim into a scratch program, compiled with this harness's own flags
// (g++ -std=c++17 -O1 -g -fsanitize=address,undefined), run on the inputs below, and its output (printf "%a") pasted here.
// Expected values per case, in order: P[0, m) as re, im pairs, R[0, m] as re, im pairs, beta.
struct NewtonRestartCase {
  const char* name;
  int m, ldh;
  int n_s;           // Leja points / coefficients of earlier restarts in front of this restart's slice
  int complex_hess;  // 0: real Hessenberg entries (imaginary parts exactly zero)
  int nu_mode;       // 0: no nu (orthonormal basis); 1: nu near one; 2: as 1, with nu[zero_at] = 0
  int zero_at;
  unsigned long long seed;
  double radius, beta;
};
static const NewtonRestartCase kNewtonRestartCases[] = {
  {"m = 1: no polynomial loop, complex", 1, 2, 0, 1, 0, 0, 11, 2.5, 0.75},
  {"m = 1 after earlier restarts, stored basis", 1, 4, 3, 1, 1, 0, 12, 1.75, 1.25},
  {"m = 2, real Hessenberg matrix", 2, 3, 0, 0, 0, 0, 13, 3.0, 1.0},
  {"m = 2, complex, n_s = 2, nu", 2, 5, 2, 1, 1, 0, 14, 2.25, 0.5},
  {"m = 3, complex, first restart", 3, 4, 0, 1, 0, 0, 15, 2.5, 2.0},
  {"m = 3, real, n_s = 6, nu with nu[3] = 0 (the vector of a breakdown at norm 0)", 3, 8, 6, 0, 2, 3, 16, 4.0, 0.875},
  {"m = 7, complex, first restart, ldh = m_max + 1 = 13", 7, 13, 0, 1, 0, 0, 17, 3.5, 1.0},
  {"m = 7, complex, n_s = 7, nu", 7, 8, 7, 1, 1, 0, 18, 3.5, 0.0625},
  {"m = 7, real, n_s = 14, nu with nu[2] = 0", 7, 8, 14, 0, 2, 2, 19, 2.75, 1.5},
  {"m = 20, complex, first restart", 20, 21, 0, 1, 0, 0, 20, 5.0, 1.0},
  {"m = 20, real, n_s = 20", 20, 21, 20, 0, 0, 0, 21, 5.0, 0.25},
  {"m = 20, complex, n_s = 40, nu, ldh = 24", 20, 24, 40, 1, 1, 0, 22, 6.0, 0.125},
};
// The inputs of a case, from its seed: every value is an integer in [-2000, 2000] over 1024 (nu: 1 + integer / 2^20), exact in
// binary floating point on every platform.  Hess is upper Hessenberg in its first m columns ((m + 1) x m, leading dimension ldh),
// everything else is zero, as newton! leaves it.  a and leja have n_s + m entries; the restart's slice starts at n_s.
struct NewtonRestartInputs {
  std::vector<std::complex<double>> Hess, a, leja;
  std::vector<double> nu;
};
static inline NewtonRestartInputs newton_restart_inputs(const NewtonRestartCase& c) {
  unsigned long long x = c.seed;
  auto next = [&x]() {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    return (double)((long long)((x >> 33) % 4001ull) - 2000) / 1024.0;
  };
  NewtonRestartInputs in;
  in.Hess.assign((size_t)c.ldh * c.ldh, std::complex<double>(0));
  for (int k = 0; k < c.m; ++k)
    for (int i = 0; i <= k + 1; ++i) {
      const double re = next(), im = next();
      in.Hess[(size_t)k * c.ldh + i] = std::complex<double>(re, c.complex_hess ? im : 0.0);
    }
  for (int i = 0; i < c.n_s + c.m; ++i) {
    const double ar = next(), ai = next(), lr = next(), li = next();
    in.a.push_back(std::complex<double>(ar, ai));
    in.leja.push_back(std::complex<double>(lr, li));
  }
  if (c.nu_mode) {
    for (int i = 0; i <= c.m; ++i) in.nu.push_back(1.0 + next() / 1024.0);
    if (c.nu_mode == 2) in.nu[c.zero_at] = 0.0;
  }
  return in;
}
static const double kNewtonRestartExpected[] = {
  // m = 1: no polynomial loop, complex: P[0, 1), R[0, 1], beta
  0x1.aap-1, 0x1.7dp-1,
  0x1.173a0d25c6594p-2, -0x1.135dd1fac8534p-1, 0x1.95c21251a1ffep-1, 0x1.76049d9aceb28p-4,
  0x1.661be3745b047p-1,
  // m = 1 after earlier restarts, stored basis: P[0, 1), R[0, 1], beta
  -0x1.092eb3abfc651p+0, -0x1.d35854230d862p+0,
  0x1.671295372df01p-1, -0x1.2be8fe4602083p-2, -0x1.f3e8e48490781p-2, 0x1.b4cfd4f0e07bdp-2,
  0x1.64636a7cc340ap+1,
  // m = 2, real Hessenberg matrix: P[0, 2), R[0, 2], beta
  -0x1.f966aaaaaaaa8p-3, -0x1.a243555555556p-1, 0x1.15a1p+0, -0x1.7ddp-2,
  -0x1.693a32db37d69p-1, -0x1.0903117efc93dp-4, 0x1.d16eca491cc1bp-3, -0x1.233338dd52ff4p-1, -0x1.670661f561afdp-2, 0x0p+0,
  0x1.e9297513f8fd6p-1,
  // m = 2, complex, n_s = 2, nu: P[0, 2), R[0, 2], beta
  0x1.27c25bf7f61c6p-3, -0x1.0ab07e76a8d3p-1, 0x1.d95c853efc264p-2, -0x1.d0b279fe5ee4ep-2,
  -0x1.241727e2124a9p-2, 0x1.c9419c9f322ep-3, 0x1.7bf7d464bc1e8p-2, -0x1.f5804778b2768p-2, -0x1.4026c117b4e8fp-1, -0x1.44448a976932cp-2,
  0x1.77f07b0d5afd2p-2,
  // m = 3, complex, first restart: P[0, 3), R[0, 3], beta
  0x1.9b895920a3d71p+1, 0x1.19b790a99999ap+1, 0x1.5ba1445666666p+2, -0x1.7960e7c28f5c2p-2, -0x1.278664428f5c4p-2, 0x1.19019d4666666p+0,
  0x1.a7b5335d5dbe5p-2, 0x1.5ac872854e244p-2, 0x1.8a1302dd171cp-1, -0x1.150f8c52e41fcp-2, 0x1.c7ba2a4f8e41ep-4, 0x1.103f671b2ddbp-5, 0x1.9118d25d42219p-4, -0x1.4686f83c39fc1p-3,
  0x1.8d5c850b28521p+1,
  // m = 3, real, n_s = 6, nu with nu[3] = 0 (the vector of a breakdown at norm 0): P[0, 3), R[0, 3], beta
  -0x1.80820e71ffc8dp+0, 0x1.bc2e4f25f97a8p-1, 0x1.5ed141260cd76p-2, -0x1.3bcfa0d805adfp-2, 0x1.c606d3ffe4083p-6, 0x1.805ff662d10ccp-7,
  0x1.f71363e21f5f5p-2, 0x1.39f82e4b81018p-1, -0x1.4250dc7253a51p-2, -0x1.fdc4f376ea168p-2, -0x1.ac3b968676482p-4, -0x1.022026c75b58cp-3, 0x0p+0, 0x0p+0,
  0x1.bd7da45c25c38p-3,
  // m = 7, complex, first restart, ldh = m_max + 1 = 13: P[0, 7), R[0, 7], beta
  -0x1.37a4a42599423p-2, -0x1.e05f028d05828p+0, 0x1.ef02e60550d25p+0, 0x1.1fffdff867037p+1, 0x1.87f3f1148bf62p-1, 0x1.f0cb7565c0adp-2, 0x1.323e3d6c87916p-4, 0x1.02ab04781a921p-2, 0x1.545750a871a28p-3, -0x1.8eef6525dbc17p-5, -0x1.2443904a89189p-5, -0x1.36afd9a3a63dap-6, -0x1.2b03b89056a07p-7, -0x1.4b4a3fbf9884p-8,
  0x1.cfc028bfe27fap-8, -0x1.aa2469fe5ab83p-2, -0x1.b077631c68e88p-2, 0x1.77859ab24bb29p-1, -0x1.d68cb289cc445p-5, 0x1.a3b0ba3fb0deap-3, -0x1.65b7707ce291ep-3, 0x1.7436ba40ebf61p-6, -0x1.f5407f4d57618p-5, 0x1.5ce33ac2199bfp-3, 0x1.f7310af6eb5a7p-6, -0x1.8745a0cf8d6b7p-11, -0x1.3e8a6855a83ap-7, 0x1.e7e352b8bfe2fp-7, -0x1.9d58e8c2448ffp-8, -0x1.2a4352b3b4eeap-7,
  0x1.a359131680b0ep-3,
  // m = 7, complex, n_s = 7, nu: P[0, 7), R[0, 7], beta
  -0x1.288eea135a86ap-5, -0x1.a1bca81f90a94p-5, 0x1.a746034efdafcp-5, 0x1.4cef6c9b84f31p-5, 0x1.3cb676d868693p-8, 0x1.6549ef8cd297fp-7, 0x1.780b138892033p-8, -0x1.c91d61f65549ep-14, -0x1.f0c6cf83d3b9ep-12, 0x1.a41545b73ecafp-10, 0x1.e6ae644f0fa1dp-11, 0x1.a3fde0f0a219ep-10, -0x1.458e960f31165p-11, -0x1.8e969c6e371b8p-13,
  -0x1.9d14879d0182ep-3, -0x1.1db4756b93002p-2, -0x1.7f334593ecdbap-1, -0x1.c08756b3ec274p-2, -0x1.98b1315817bebp-3, -0x1.b6dae4a4a39b5p-3, -0x1.f37b7312bbc46p-4, 0x1.18a05ef499885p-3, -0x1.7fe70589ce5a4p-4, 0x1.aaa9a2d6b83c5p-9, 0x1.060e7eebe121bp-5, 0x1.90562915afb4cp-6, -0x1.6a1887ec23c23p-7, 0x1.7121ef3466c77p-6, 0x1.3106aa553f2c7p-8, -0x1.ca32a8a628cc8p-10,
  0x1.4f47e1e1644b4p-5,
  // m = 7, real, n_s = 14, nu with nu[2] = 0: P[0, 7), R[0, 7], beta
  0x1.3fba5bb6a008p-3, -0x1.45803362b0ebep+0, -0x1.0f880669a2d68p-2, -0x1.47d7c9be8fdc1p-1, -0x0p+0, -0x0p+0, -0x1.68a8978a14cd5p-6, -0x1.72317918518c7p-7, -0x1.652c76c76f416p-7, -0x1.131158683646fp-8, -0x1.ad9aa98e42c67p-8, -0x1.15987d18821ffp-8, 0x1.dffeb2fd8dfb7p-14, 0x1.ad86b1097ac77p-13,
  0x1.c280349c9cb3bp-5, -0x1.4b8da592fdae1p-5, 0x1.245e305b4efa6p-3, 0x1.b591d3df429cp-4, 0x0p+0, -0x0p+0, 0x1.04e58e359f882p-3, -0x1.06b3f4789c80bp-2, 0x1.3c5ab1484e852p-3, -0x1.f6367d0d918a4p-4, 0x1.3385ba4ec5916p-3, -0x1.1311f56bea2c9p-4, -0x1.eb7e990b97e4fp-8, 0x1.b69d18239fc18p-10, 0x1.6fa1a1bc65856p-10, 0x0p+0,
  0x1.083f07d0f93fdp-5,
  // m = 20, complex, first restart: P[0, 20), R[0, 20], beta
  0x1.1f24dbb93462cp+1, 0x1.02f50800f0438p+1, 0x1.5978ecb170c2bp-2, -0x1.ddc2b30d8b1dcp-2, 0x1.6d7b36e4c62dep-3, -0x1.9e4e8a952492bp-3, 0x1.36d46c8f9f4e1p-5, -0x1.3238d4a48f01bp-7, 0x1.5d8bbb557f945p-7, 0x1.078d6576fefdcp-7, 0x1.738778f6ce8d2p-11, -0x1.6a1b002c0f78p-10, -0x1.806f81a56de32p-10, 0x1.53d53aba17fa5p-14, 0x1.b28d0439988dcp-13, -0x1.7cca24280d2bcp-15, 0x1.d5645ffb90e06p-16, 0x1.4d3fd82e4ff85p-16, 0x1.d70827bb345cap-19, -0x1.c4237d5eacebep-17, -0x1.f08638f851b1ep-19, -0x1.4bb73b92bf20ap-17, 0x1.9b4884d22a78dp-21, -0x1.a71b43d28c868p-19, -0x1.ae4ac89eb2dcp-20, 0x1.46c896570b902p-21, 0x1.501a8bc2581dp-23, 0x1.9ed8712a9d7bcp-22, -0x1.60ce38e69530cp-24, 0x1.230f717ce3fecp-26, 0x1.192f09e5a1c67p-25, 0x1.0d950efaf29cdp-25, -0x1.71c00a2b22133p-28, -0x1.4987bda5935bap-32, 0x1.10979d97c6b6bp-30, 0x1.48403c919311ap-30, -0x1.24e82d943fcedp-32, 0x1.a2a9b34ef000bp-33, -0x1.b16b606580697p-37, -0x1.2d3d50e4b77f7p-38,
  -0x1.008cbde7dc45ap-2, -0x1.89a8e28de0264p-1, -0x1.f0c1030aae1dfp-2, 0x1.3447848a15aacp-3, -0x1.eec99656d50e1p-3, 0x1.4756959f3604fp-3, -0x1.b092a985ecd56p-5, -0x1.89e2534d68f66p-6, 0x1.68f61273efbc5p-10, -0x1.5ecac1c993fccp-6, -0x1.27803d9c4b95fp-9, 0x1.c5e7de53403dcp-7, -0x1.bf08445cdd2b5p-9, -0x1.64246a1c7af2p-7, -0x1.8a924830c0761p-9, 0x1.ea953c19688cp-10, -0x1.dace05a67bab6p-13, -0x1.2a9bd77985ebep-10, 0x1.61fc75018e679p-11, 0x1.5e613f6d63014p-11, -0x1.14af8ac6291fep-11, -0x1.d41552f4f2ea9p-12, -0x1.87af2d8ca77edp-12, 0x1.fb95769c6d35p-12, -0x1.190dc53478bd5p-12, -0x1.699cb083fe553p-13, 0x1.fedf5ae016e4p-14, -0x1.625eab0446b5cp-16, 0x1.28826789c2fb1p-16, -0x1.19f9eb33d04b4p-15, -0x1.5ccc99c8e400fp-18, 0x1.e5bfb0719f6dp-22, -0x1.3cc40f29e3d33p-20, 0x1.4bde5ecca6b79p-20, 0x1.74b731f9e0b6dp-20, 0x1.a0d9998dd1eb1p-20, 0x1.2c334067471a5p-24, 0x1.8d514c4513331p-21, -0x1.5121c73f77c1dp-25, 0x1.4712031a4d0bep-25, 0x1.f9617abee2173p-28, 0x1.320de551e3b71p-31,
  0x1.389cef49ce5ecp-12,
  // m = 20, real, n_s = 20: P[0, 20), R[0, 20], beta
  -0x1.31a5a56a8fedcp-1, 0x1.959904e783abdp-7, -0x1.c1d8cdef37344p-6, -0x1.bac8ef65d197cp-6, -0x1.535a25800925bp-8, 0x1.2b49684302bebp-7, -0x1.cd81759794329p-13, 0x1.f216defe9fec1p-11, -0x1.c1ed5cab1dbcfp-14, 0x1.06f5607ce7c42p-12, -0x1.90a97086bc928p-17, 0x1.7766dbbda8c86p-15, 0x1.6213727e3312dp-22, 0x1.f8d06da4d9686p-24, 0x1.fea8a919074ep-24, -0x1.d4c372584135bp-22, -0x1.f966e776da9f4p-24, -0x1.c43d389dec263p-24, 0x1.773827f84db4fp-28, 0x1.75cde364b23afp-26, 0x1.05831c0bb31f8p-30, -0x1.6d1ef6e613789p-28, 0x1.a0ae7a472b821p-30, 0x1.69bcb50e31be4p-31, -0x1.5e25494740f6ep-31, 0x1.bc87ee11943b7p-31, -0x1.d80fd13ee52bep-35, -0x1.9fcd3d7604c5fp-34, 0x1.a3c9e2b72cd36p-35, 0x1.19863ab5b04dep-37, -0x1.1574865d2ee84p-38, -0x1.5786ee1340835p-39, -0x1.d06038d52fda6p-41, -0x1.4e69b0c03771ap-42, -0x1.20011f01dc65ep-45, -0x1.b8d41ad05355p-44, 0x1.82ee5e6c3b85ap-47, 0x1.26cc5ef7597ccp-50, -0x1.71d8e6d3ffb37p-56, -0x1.e0a799b301a4ap-53,
  0x1.ad26fb6d90884p-2, -0x1.dc0032456e6ddp-3, -0x1.1289cef595903p-3, 0x1.3131466e85249p-4, 0x1.b9104d9633c67p-3, -0x1.e99c3b0bb0e45p-4, 0x1.a181fd9ebe166p-2, -0x1.cfc2959490894p-3, 0x1.128ad13578b47p-1, -0x1.30eb2cb7e71b3p-2, 0x1.0fe920d152f4ep-2, -0x1.2de69e7fac5afp-3, -0x1.74ee0ca1d8194p-7, 0x1.9b5d17e73bc42p-8, -0x1.2513efb40c4fep-8, 0x1.4740c4aa04004p-9, -0x1.736e917a15275p-10, 0x1.8123aacfcd34cp-11, 0x1.00532cfce1027p-12, -0x1.052ae74c32d6ep-12, -0x1.7e45195454bb5p-13, -0x1.8f71e8edd8ce3p-19, 0x1.3d468dadb6f84p-14, -0x1.6cad9cea537cap-13, 0x1.70cf033b4531ap-15, 0x1.40b019a13c799p-15, -0x1.7579227566494p-15, 0x1.a1a8d496be4c8p-15, -0x1.fd02943f66b26p-17, 0x1.1bdf7ea6d9692p-18, 0x1.c68d0a5e4b3p-20, -0x1.aefe1d60968dfp-20, 0x1.73a9b28d10f87p-22, -0x1.0bf4068dec086p-24, 0x1.fab9b7fa4fc88p-25, -0x1.30fc00e3a67d7p-23, -0x1.6f3c810611f8dp-25, -0x1.4e1e470cf0414p-28, 0x1.7505b5b1792d9p-32, -0x1.744a7798877eep-30, -0x1.f8f844defb94fp-33, 0x0p+0,
  0x1.00d7bb1f3dd69p-22,
  // m = 20, complex, n_s = 40, nu, ldh = 24: P[0, 20), R[0, 20], beta
  0x1.1eded0186994p-4, -0x1.9b064383a4a47p-4, -0x1.cb04d803d045fp-7, -0x1.561ba7b91becbp-13, 0x1.5365c97c285fap-8, 0x1.2a057826f6b5ep-7, -0x1.c1c98749fe2p-10, -0x1.97c994ecf5863p-10, 0x1.cb009654bd168p-14, -0x1.5381823a4d3adp-12, -0x1.0c8f5a77e15a7p-14, -0x1.ed71bfca08742p-15, -0x1.05ae4ca001fe1p-15, -0x1.0edd22bbacd1fp-17, -0x1.b28e60b182756p-18, -0x1.f45018a2c828fp-18, -0x1.7fd2a96068f4ep-19, -0x1.daf40bd12f57fp-23, -0x1.29740d38f2fd2p-23, -0x1.07b35c0786c22p-24, -0x1.0587a9238fc2fp-24, -0x1.69108d7a53417p-25, 0x1.2ecb1c9b29758p-26, -0x1.516566fd90901p-26, 0x1.160cba356f94p-31, -0x1.b0b81c9592681p-31, -0x1.adfdca0be485cp-35, 0x1.333e2e7a96a18p-33, 0x1.fe985d26f7304p-36, 0x1.65132f2a5f849p-37, -0x1.642e9ab1e76cbp-40, 0x1.39ef8f3b2db64p-38, -0x1.15b37ecb8ac3p-39, -0x1.8e3f95e8bb0f6p-40, 0x1.9539939b8c233p-43, -0x1.19fdaf9a48477p-41, -0x1.226120cc834ap-44, -0x1.6ea02497cc515p-46, -0x1.559d9f969f8e1p-50, -0x1.3a69aac6b179ap-51,
  -0x1.769986a6523b6p-4, -0x1.6e1c19041d56p-2, -0x1.a55b29c76ce1ap-5, -0x1.99d503dded82bp-2, 0x1.21238b9c1ab34p-3, 0x1.eca05ae88faaap-2, -0x1.dc4ad9730a1a4p-3, -0x1.8cfa7de476893p-3, 0x1.63c5bbf58b4b5p-2, -0x1.ca4a41035dcd3p-3, -0x1.2f8fb0bf4dcfdp-3, -0x1.39469aa8f32f2p-2, -0x1.88773df40259bp-3, -0x1.4168724e14c24p-4, 0x1.d6b20c6142314p-6, -0x1.eda38d51cbbfdp-4, 0x1.47cf34365cb8bp-6, -0x1.c5f933aa13281p-4, 0x1.9c049174ed392p-6, -0x1.207b3acacc737p-7, 0x1.9d8898ff3827dp-7, 0x1.0315ff7b9dd67p-8, -0x1.2cb5a4205ab2p-11, 0x1.5392288e486f7p-8, 0x1.ad7a3e443087p-13, 0x1.0c462ec98a4edp-12, -0x1.a77fdd5788286p-14, -0x1.3e80cc1f4a7fep-14, -0x1.2824482d000bdp-15, 0x1.0b9e4b6d69e99p-16, 0x1.5afc047540998p-21, -0x1.1dbeb7bcb8f8ep-17, 0x1.2d0b0286206a1p-17, -0x1.8d8da5eafc474p-19, 0x1.8cd19a85cc06ep-19, 0x1.925a3e1148935p-18, 0x1.b231d9e12b9acp-20, -0x1.33f0912562b56p-20, 0x1.5334f8d609caap-24, -0x1.12a2b6fdd1a45p-24, -0x1.76461ae8f4a0ep-27, -0x1.037b577a1cae6p-27,
  0x1.6839bd586631p-27,
};
