"""The parametrisation shared by the CPU and GPU halves of the primitive-level tests."""
import prims_cases as K

MAPS = ["ident", "stride", "split"]
WSUM_NIN = [1, 2, 79, 80]
WSUM_NOUT = [1, 8, 9]
KINDS = ["qm1", "half", "uniform"]
RESCALE_ELL = [2, 3, 7]
CONV = K.conv_shapes()
