// pt_deform.hip -- linear blend skinning for the device (pt_skin.h; include/pt_deform.h): the kernel and its launch are
// pt_deform_kernels.h; and blend shapes in front of it (pt_morph_skin.h; include/pt_morph.h): pt_morph_kernels.h, which
// uses the former's loads and dot and therefore shares this unit.  Compiled with -ffp-contract=off like the rest: every product and sum
// is the IEEE operation of the host code.
#include "pt_deform_kernels.h"
#include "pt_morph_kernels.h"
