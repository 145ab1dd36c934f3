// pt_deform.hip -- linear blend skinning for the device (pt_skin.h; include/pt_deform.h): the kernel and its launch are
// pt_deform_kernels.h.  Compiled with -ffp-contract=off like the rest: every product and sum is the IEEE operation of the host code.
#include "pt_deform_kernels.h"
