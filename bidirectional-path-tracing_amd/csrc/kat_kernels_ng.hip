// The per-function BSDF kernel as bdpt_kernels_ng.hip compiles its device functions:
// the same source as kat_kernels.hip with BDPT_GLOSSY 0 and the fast weights of the
// frame kernels. For material tables of diffuse, mirror and glass records only (the
// host refuses any other, bdpt_capi.cpp). Only the BSDF kernel and its launcher, with
// an _ng name.
#define BDPT_GLOSSY 0
#define BDPT_FAST_WEIGHTS 1
#define KAT_VARIANT _ng
#include "kat_kernels.hip"
