// Run-time-signature row-tile kernels (cemlp_sig.hpp) for the algebras with 5 generators: every signature, float and double.
#define CSMPN_SIG_N 5
#include "sig_inst.inc"
