// Run-time-signature row-tile kernels (cemlp_sig.hpp) for the algebras with 2 generators: every signature, float and double.
#define CSMPN_SIG_N 2
#include "sig_inst.inc"
