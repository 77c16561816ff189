"""ctypes mirrors of the C structs in include/dogleg.h and include/dlg_trace.h.

Plumbing shared by the product bindings (capi.py) and by the tests' oracle
bindings.  Layouts follow include/dogleg.h, which follows the reference
(/root/reference/dogleg.h:48-210).
"""
import ctypes as C
import numpy as np

DOGLEG_DEBUG_VNLOG_BIT = 30
DOGLEG_DENSE, DOGLEG_SPARSE, DOGLEG_DENSE_PRODUCTS = 0, 1, 2
STEP_NAMES = {0: "cauchy", 1: "gaussnewton", 2: "interpolated"}


class Parameters2(C.Structure):
    """dogleg_parameters2_t (reference dogleg.h:112-152)."""
    _fields_ = [
        ("max_iterations", C.c_int),
        ("dogleg_debug", C.c_int),  # bit0 debug, bit1 JtJ_packed, bit2 JtJ_upper, bit30 vnlog
        ("trustregion0", C.c_double),
        ("trustregion_decrease_factor", C.c_double),
        ("trustregion_decrease_threshold", C.c_double),
        ("trustregion_increase_factor", C.c_double),
        ("trustregion_increase_threshold", C.c_double),
        ("Jt_x_threshold", C.c_double),
        ("update_threshold", C.c_double),
        ("trustregion_threshold", C.c_double),
    ]

    def _bit(self, b, v=None):
        if v is None:
            return bool((self.dogleg_debug >> b) & 1)
        if v:
            self.dogleg_debug |= (1 << b)
        else:
            self.dogleg_debug &= ~(1 << b)

    debug = property(lambda s: s._bit(0), lambda s, v: s._bit(0, v))
    JtJ_packed = property(lambda s: s._bit(1), lambda s, v: s._bit(1, v))
    JtJ_upper = property(lambda s: s._bit(2), lambda s, v: s._bit(2, v))
    debug_vnlog = property(lambda s: s._bit(DOGLEG_DEBUG_VNLOG_BIT),
                           lambda s, v: s._bit(DOGLEG_DEBUG_VNLOG_BIT, v))


class CholmodSparse(C.Structure):
    """cholmod_sparse as far as a dogleg callback touches it."""
    _fields_ = [
        ("nrow", C.c_size_t), ("ncol", C.c_size_t), ("nzmax", C.c_size_t),
        ("p", C.c_void_p), ("i", C.c_void_p), ("nz", C.c_void_p),
        ("x", C.c_void_p), ("z", C.c_void_p),
        ("stype", C.c_int), ("itype", C.c_int), ("xtype", C.c_int),
        ("dtype", C.c_int), ("sorted", C.c_int), ("packed", C.c_int),
    ]


class Trial(C.Structure):
    """dlg_trial_t (include/dlg_trace.h)."""
    _fields_ = [
        ("iteration", C.c_int), ("accepted", C.c_int),
        ("step_type", C.c_int), ("did_step_to_edge", C.c_int),
        ("norm2x_before", C.c_double), ("norm2x_after", C.c_double),
        ("norm2_cauchy", C.c_double), ("norm2_gn", C.c_double),
        ("k_cauchy_to_gn", C.c_double), ("norm2_step", C.c_double),
        ("expected_improvement", C.c_double), ("observed_improvement", C.c_double),
        ("rho", C.c_double),
        ("trustregion_before", C.c_double), ("trustregion_after", C.c_double),
        ("lambda_", C.c_double),
    ]

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Trace(C.Structure):
    """dlg_trace_t (include/dlg_trace.h)."""
    _fields_ = [
        ("capacity", C.c_int), ("ntrials", C.c_int),
        ("ncallbacks", C.c_int), ("nstate", C.c_int),
        ("trials", C.POINTER(Trial)),
        ("p_trial", C.POINTER(C.c_double)),
        ("step", C.POINTER(C.c_double)),
    ]


class TraceBuffer:
    """Owns the arrays a dlg_trace_t points at."""

    def __init__(self, nstate, capacity=256):
        self.capacity = capacity
        self.nstate = nstate
        self._trials = (Trial * capacity)()
        self.p_trial = np.zeros((capacity, nstate), dtype=np.float64)
        self.step = np.zeros((capacity, nstate), dtype=np.float64)
        self.c = Trace(capacity, 0, 0, nstate,
                       C.cast(self._trials, C.POINTER(Trial)),
                       self.p_trial.ctypes.data_as(C.POINTER(C.c_double)),
                       self.step.ctypes.data_as(C.POINTER(C.c_double)))

    def byref(self):
        return C.byref(self.c)

    @property
    def ntrials(self):
        return min(self.c.ntrials, self.capacity)

    @property
    def ncallbacks(self):
        return self.c.ncallbacks

    def trials(self):
        return [self._trials[i].asdict() for i in range(self.ntrials)]


BATCH_JTX, BATCH_SMALL_STEP, BATCH_TRUSTREGION, BATCH_MAX_ITERATIONS, BATCH_FAILED = 1, 2, 3, 4, 5
BATCH_MAX_NSTATE = 64
BATCH_UNC_OK, BATCH_UNC_FAILED = 0, 1            # dogleg_amd_dense_batch_uncertainty's status
BATCH_NOT_RUN, BATCH_UNC_SKIPPED = 0, 2          # the device-resident entry points: a problem whose active byte is 0
BATCH_QUERY_MAX_ROWS = 16                        # dogleg_amd_dense_batch_query_covariance: rows of a query


class BatchResult(C.Structure):
    """dogleg_amd_batch_result_t (include/dogleg.h)."""
    _fields_ = [
        ("norm2_x", C.c_double), ("trustregion", C.c_double), ("lambda_", C.c_double),
        ("iterations", C.c_int), ("evaluations", C.c_int), ("status", C.c_int),
    ]


LOSS_TRIVIAL, LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY = 0, 1, 2, 3      # dogleg_amd_batch_loss_t.kind
BATCH_LOSS_MAX_FEATURESIZE = 4


class BatchLoss(C.Structure):
    """dogleg_amd_batch_loss_t (include/dogleg.h)."""
    _fields_ = [("kind", C.c_int), ("scale", C.c_double), ("featureSize", C.c_int)]


class BatchBounds(C.Structure):
    """dogleg_amd_batch_bounds_t (include/dogleg.h): three addresses, each 0 for NULL."""
    _fields_ = [("lower", C.c_void_p), ("upper", C.c_void_p), ("held", C.c_void_p)]


class BatchFit(C.Structure):
    """dogleg_amd_batch_fit_t (include/dogleg.h): a BatchLoss* and two addresses, each 0 for NULL."""
    _fields_ = [("loss", C.POINTER(BatchLoss)), ("weights", C.c_void_p), ("held", C.c_void_p)]


MODEL_EXPDECAY, MODEL_GAUSS1D, MODEL_GAUSS2D, MODEL_GAUSS2D_ELLIPTIC = 0, 1, 2, 3      # dogleg_amd_batch_model_t.kind
MODEL_NSTATE = {MODEL_EXPDECAY: 3, MODEL_GAUSS1D: 4, MODEL_GAUSS2D: 5, MODEL_GAUSS2D_ELLIPTIC: 6}
LIKELIHOOD_GAUSS, LIKELIHOOD_POISSON = 0, 1        # dogleg_amd_optimize_dense_batch_model_mle


class BatchModel(C.Structure):
    """dogleg_amd_batch_model_t (include/dogleg.h): y, t and scale are device addresses, each 0 for NULL."""
    _fields_ = [("kind", C.c_int), ("Nmeas", C.c_uint), ("width", C.c_uint), ("height", C.c_uint),
                ("y", C.c_void_p), ("t", C.c_void_p), ("scale", C.c_void_p), ("t_per_problem", C.c_int)]


DATA_F64, DATA_F32, DATA_U16 = 0, 1, 2        # dogleg_amd_batch_camera_t.dtype
DATA_NUMPY = {DATA_F64: "float64", DATA_F32: "float32", DATA_U16: "uint16"}


class BatchCamera(C.Structure):
    """dogleg_amd_batch_camera_t (include/dogleg.h): the model record (y 0) and the camera's data; raw, the three maps and origin
    are device addresses, each 0 for NULL."""
    _fields_ = [("model", BatchModel), ("dtype", C.c_int), ("raw", C.c_void_p),
                ("sensor_width", C.c_uint), ("sensor_height", C.c_uint),
                ("offset", C.c_void_p), ("gain_inv", C.c_void_p), ("readvar", C.c_void_p), ("origin", C.c_void_p)]


class JacobianReport(C.Structure):
    """dogleg_amd_jacobian_report_t (include/dogleg.h)."""
    _fields_ = [
        ("nchecked", C.c_longlong), ("nbad", C.c_longlong), ("nnonfinite", C.c_longlong), ("noutside", C.c_longlong),
        ("max_error", C.c_double), ("max_error_relative", C.c_double),
        ("worst_var", C.c_int), ("worst_meas", C.c_int), ("worst_reported", C.c_double), ("worst_observed", C.c_double),
        ("ncolours", C.c_int), ("evaluations", C.c_int),
    ]

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class JacobianEntry(C.Structure):
    """dogleg_amd_jacobian_entry_t (include/dogleg.h)."""
    _fields_ = [("problem", C.c_int), ("var", C.c_int), ("meas", C.c_int), ("reported", C.c_double), ("observed", C.c_double)]

    def astuple(self):
        return (self.problem, self.var, self.meas, self.reported, self.observed)


JACOBIAN_ONE_AT_A_TIME = 1

NUMERIC_FORWARD, NUMERIC_CENTRAL = 0, 1          # dogleg_amd_numeric_options_t.scheme
NUMERIC_DELTA_DEFAULT = {NUMERIC_FORWARD: 2.0 ** -26, NUMERIC_CENTRAL: 2.0 ** -17}     # of delta_rel and of delta_abs
NUMERIC_TILE_ROWS = 32                           # rows of J per tile of k_numeric_jacobian (csrc/batch_numeric.hip: NUM_TR)


class NumericOptions(C.Structure):
    """dogleg_amd_numeric_options_t (include/dogleg.h): lower / upper are addresses, each 0 for NULL."""
    _fields_ = [("scheme", C.c_int), ("delta_rel", C.c_double), ("delta_abs", C.c_double),
                ("lower", C.c_void_p), ("upper", C.c_void_p), ("bounds_on_device", C.c_int)]


# dogleg_callback_device_batch_t
CB_DEVICE_BATCH = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p)
# dogleg_callback_device_batch_products_t
CB_DEVICE_BATCH_PRODUCTS = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p,
                                       C.c_void_p)

# dogleg_callback_device_batch_values_t
CB_DEVICE_BATCH_VALUES = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p)

# dogleg_callback_device_values_t
CB_DEVICE_VALUES = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p)
# csrc/numeric_device.hip: rows of a tile of k_numeric_jacobian_sparse (ND_TR), the copies one LDS chunk stages at most
# (ND_SLOTS: copy 0 and the chunk's plus and minus copies), the lanes of a workgroup (ND_THREADS), and the dense tile's edge
NUMERIC_DEVICE_TILE_ROWS, NUMERIC_DEVICE_LDS_SLOTS, NUMERIC_DEVICE_THREADS, NUMERIC_DEVICE_DENSE_TILE = 64, 63, 256, 32

CB_SPARSE = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double),
                        C.POINTER(CholmodSparse), C.c_void_p)
CB_DENSE = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double),
                       C.POINTER(C.c_double), C.c_void_p)
CB_PRODUCTS = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double),
                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)


def dptr(a):
    """double* of a C-contiguous float64 numpy array."""
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_double))


def iptr(a):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_int))
