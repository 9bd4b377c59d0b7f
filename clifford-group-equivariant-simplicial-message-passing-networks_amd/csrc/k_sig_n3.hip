// Run-time-signature row-tile kernels (cemlp_sig.hpp) for the algebras with 3 generators: every signature, float and double.
#define CSMPN_SIG_N 3
#include "sig_inst.inc"
