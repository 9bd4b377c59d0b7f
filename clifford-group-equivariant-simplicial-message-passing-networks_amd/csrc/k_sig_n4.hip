// Run-time-signature row-tile kernels (cemlp_sig.hpp) for the algebras with 4 generators: every signature, float and double.
#define CSMPN_SIG_N 4
#include "sig_inst.inc"
