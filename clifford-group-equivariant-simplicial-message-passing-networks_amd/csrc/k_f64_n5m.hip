// Float64 row-tile kernels (cemlp_f64.hpp) for the algebra with 5 generators, negative-signature mask 0x10u.
#define CSMPN_ALG_N 5
#define CSMPN_ALG_NEG 0x10u
#define CSMPN_ALG_TAG n5m
#include "f64_inst.inc"
