// The persistent phase machine's kernels with forced frames (PmForce, persist.h) and their launcher, pm_launch_forced: the
// text of persist.hip compiled with FRC = true, in a translation unit of its own (see the PM_FORCED_TU section there).
#define PM_FORCED_TU 1
#include "persist.hip"
