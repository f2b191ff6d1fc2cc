// The probe variants of the production kernels (gemm_planes.hip, gemm_tn.hip, chebtile.hip) are compiled in by these macros;
// several of them compute wrong results on purpose (only their time is read).  A library built with one of them is a probe
// library: the tools/ scripts that build those say so with -DP2M_PROBE_BUILD, and any other build that defines one stops here.
#pragma once
#ifndef P2M_PROBE_BUILD
#ifdef P2M_PL_ABL_NOSTORE
#error "P2M_PL_ABL_NOSTORE builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_PL_ABL_NOLOAD
#error "P2M_PL_ABL_NOLOAD builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_PL_ABL_NOSLICE
#error "P2M_PL_ABL_NOSLICE builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_PL_ABL_NOMFMA
#error "P2M_PL_ABL_NOMFMA builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_TN_ABL_NOLOAD
#error "P2M_TN_ABL_NOLOAD builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_TN_ABL_NOSLICE
#error "P2M_TN_ABL_NOSLICE builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_TN_ABL_NOMFMA
#error "P2M_TN_ABL_NOMFMA builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_TN_TRACE
#error "P2M_TN_TRACE builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_K1_TRACE
#error "P2M_K1_TRACE builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_TILE_TRACE
#error "P2M_TILE_TRACE builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_ABL_NO_XU
#error "P2M_ABL_NO_XU builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_ABL_NO_P0
#error "P2M_ABL_NO_P0 builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_ABL_NO_CONV
#error "P2M_ABL_NO_CONV builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_ABL_LINEAR_X
#error "P2M_ABL_LINEAR_X builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_ABL_LINEAR_LT
#error "P2M_ABL_LINEAR_LT builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#ifdef P2M_ABL_LINEAR_A
#error "P2M_ABL_LINEAR_A builds a probe variant of the kernels: define P2M_PROBE_BUILD as well if that is meant"
#endif
#endif  // P2M_PROBE_BUILD
