"""ctypes binding of the C-ABI in include/qle_ekf.h (libqle_ekf.so).

The shared library is built in-tree by `make -C quadrotor_landing_amd/csrc`
(or __graft_entry__.build()).  There is no fallback: if the library is missing
or a call fails, an exception is raised.
"""
import contextlib
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# QLE_LIB selects an alternative in-tree build of the same engine (kernel tuning A/B runs)
LIB_PATH = os.environ.get("QLE_LIB") or os.path.join(_HERE, "libqle_ekf.so")

QLE_OK = 0
QLE_ERR_INVALID, QLE_ERR_HIP, QLE_ERR_NOMEM, QLE_ERR_STATE, QLE_ERR_NO_DEVICE = -1, -2, -3, -4, -5
QLE_F32, QLE_F64 = 0, 1
QLE_MAX_TAGS = 16

_d, _i32, _i64, _u64 = C.c_double, C.c_int32, C.c_int64, C.c_uint64


class QleParams(C.Structure):
    """`struct qle_params` == the reference's public members (relative_pose_EKF.hpp:66-133)."""
    _fields_ = [
        ("update_freq", _d), ("measurement_freq", _d), ("measurement_delay", _d),
        ("measurement_delay_max", _d), ("dyn_measurement_delay_offset", _d),
        ("est_bias", _i32), ("limit_measurement_freq", _i32), ("corner_margin_enbl", _i32),
        ("direct_orien_method", _i32), ("multirate_ekf", _i32), ("dynamic_meas_delay", _i32),
        ("r_cov_init", _d), ("v_cov_init", _d), ("ang_cov_init", _d), ("ab_cov_init", _d), ("wb_cov_init", _d),
        ("Q_a", _d * 3), ("Q_w", _d * 3), ("Q_ab", _d * 3), ("Q_wb", _d * 3),
        ("R_r", _d * 3), ("R_ang", _d * 3),
        ("ab_static", _d * 3), ("wb_static", _d * 3),
        ("r_v_cv", _d * 3), ("q_vc", _d * 4),
        ("camera_K", _d * 9), ("camera_width", _i32), ("camera_height", _i32),
        ("n_tags", _i32), ("_pad0", _i32),
        ("tag_in_view_margin", _d),
        ("tag_widths", _d * QLE_MAX_TAGS), ("tag_positions", _d * (3 * QLE_MAX_TAGS)),
        ("small_ang_tol", _d), ("g", _d * 3),
    ]


class QleDerived(C.Structure):
    """`struct qle_derived` == what initialize_params() computes (relative_pose_EKF.cpp:87-125)."""
    _fields_ = [
        ("dT_nom", _d), ("upd_per_meas", _i32), ("num_states", _i32), ("measurement_step_delay", _i32), ("_pad0", _i32),
        ("Q", _d * 12), ("R", _d * 6), ("cov_init", _d * 15), ("q_vc", _d * 4), ("C_vc", _d * 9),
    ]


class QleSynthCfg(C.Structure):
    _fields_ = [
        ("seed", _u64), ("filter_offset", _i64),
        ("ab_true_sigma", _d), ("wb_true_sigma", _d), ("meas_noise_scale", _d), ("imu_noise_scale", _d),
        ("perturb_filter_params", _i32), ("meas_delay_ticks", _i32), ("view_scale", _d),
    ]


class QleNodeReport(C.Structure):
    """`struct qle_node_report`: what the node publishes after a tick (NODE.cpp:192-281), one per filter."""
    _fields_ = [("pose", _d * 7), ("pose_cov", _d * 36), ("vel", _d * 3), ("accel", _d * 3), ("bias", _d * 6), ("obs", _d * 7),
                ("measurement_delay_curr", _d), ("upds_since_correction", _i32), ("performed_correction", C.c_uint8),
                ("measurement_consumed", C.c_uint8), ("state_initialized", C.c_uint8), ("reserved", C.c_uint8)]


class QlePolicy(C.Structure):
    """`struct qle_policy`: how a handle launches its ticks."""
    _fields_ = [("state_policy", _i32), ("refresh_period", _i32), ("split_k64", _i32), ("block", _i32), ("coop_ticks", _i32),
                ("ring_slots", _i32), ("state_bytes", _i64), ("ring_bytes", _i64), ("record_words", _i32), ("reserved", _i32)]


class QleDeviceView(C.Structure):
    """`struct qle_device_view`: where a handle's records live in GPU memory (wave tiles)."""
    _fields_ = [("struct_size", C.c_uint32), ("device", _i32), ("stream", C.c_void_p), ("dtype", _i32), ("num_states", _i32),
                ("batch", _i64), ("padded_batch", _i64), ("state", C.c_void_p), ("state_words", _i32), ("record_words", _i32),
                ("compact", _i32), ("reserved", _i32), ("filter_params", C.c_void_p), ("ab_static", _d * 3), ("wb_static", _d * 3)]


class QleInputsView(C.Structure):
    """`struct qle_inputs_view`: the IMU and tag records of one tick of a sequence."""
    _fields_ = [("struct_size", C.c_uint32), ("has_tag", _i32), ("u", C.c_void_p), ("z", C.c_void_p)]


class QleError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"qle error {code}: {msg}")
        self.code = code


# every symbol include/qle_ekf.h declares: name -> (restype, argtypes)
_pd = C.POINTER(_d)
_pu8 = C.POINTER(C.c_uint8)
_vp = C.c_void_p
SYMBOLS = {
    "qle_last_error": (C.c_char_p, []),
    "qle_version": (C.c_char_p, []),
    "qle_device_count": (C.c_int, [C.POINTER(_i32)]),
    "qle_params_default": (C.c_int, [C.POINTER(QleParams)]),
    "qle_params_derive": (C.c_int, [C.POINTER(QleParams), C.POINTER(QleDerived)]),
    "qle_create": (C.c_int, [C.POINTER(_vp), _i64, _i32, _i32, C.POINTER(QleParams)]),
    "qle_destroy": (C.c_int, [_vp]),
    "qle_set_params": (C.c_int, [_vp, C.POINTER(QleParams)]),
    "qle_set_filter_params": (C.c_int, [_vp, _pd]),
    "qle_get_filter_params": (C.c_int, [_vp, _pd]),
    "qle_batch_size": (_i64, [_vp]),
    "qle_dtype": (_i32, [_vp]),
    "qle_num_states": (_i32, [_vp]),
    "qle_set_state": (C.c_int, [_vp, _pd, _pd]),
    "qle_get_state": (C.c_int, [_vp, _pd, _pd]),
    "qle_mark_state_written": (C.c_int, [_vp]),
    "qle_initialize_state": (C.c_int, [_vp, _pd, _i32]),
    "qle_initialize_state_masked": (C.c_int, [_vp, _pd, _pu8, _i32]),
    "qle_initialize_state_slot": (C.c_int, [_vp, _vp, _i64, _i32]),
    "qle_get_state_initialized": (C.c_int, [_vp, _pu8]),
    "qle_enable_aux": (C.c_int, [_vp, _i32]),
    "qle_get_aux": (C.c_int, [_vp, _pd, _pd]),
    "qle_predict": (C.c_int, [_vp, _pd]),
    "qle_update": (C.c_int, [_vp, _pd, _pu8]),
    "qle_step": (C.c_int, [_vp, _pd, _pd, _pu8]),
    "qle_innovation": (C.c_int, [_vp, _pd, _pu8, _pd, _pd, _pd]),
    "qle_update_gated": (C.c_int, [_vp, _pd, _pu8, _d, _pu8, _pd]),
    "qle_step_gated": (C.c_int, [_vp, _pd, _pd, _pu8, _d, _pu8, _pd]),
    "qle_enable_gating": (C.c_int, [_vp, _i32]),
    "qle_filter_update": (C.c_int, [_vp, _pd, _pd, _pu8]),
    "qle_filter_update_stamped": (C.c_int, [_vp, _pd, _pd, _pu8, _d, _pd]),
    "qle_get_measurement_delay": (C.c_int, [_vp, _pd]),
    "qle_set_uniform_measurement_age": (C.c_int, [_vp, _d]),
    "qle_get_history_info": (C.c_int, [_vp, C.POINTER(_i64), C.POINTER(_i32)]),
    "qle_get_tick_flags": (C.c_int, [_vp, _pu8, _pu8, C.POINTER(_i32)]),
    "qle_inputs_create": (C.c_int, [_vp, _i64, _pu8, C.POINTER(_vp)]),
    "qle_inputs_destroy": (C.c_int, [_vp]),
    "qle_inputs_upload_tick": (C.c_int, [_vp, _i64, _pd, _pd, _pu8]),
    "qle_inputs_download_tick": (C.c_int, [_vp, _i64, _pd, _pd, _pu8]),
    "qle_run": (C.c_int, [_vp, _vp, _i64, _i64]),
    "qle_run_resident": (C.c_int, [_vp, _vp, _i64, _i64]),
    "qle_synth_cfg_default": (C.c_int, [C.POINTER(QleSynthCfg)]),
    "qle_synth_generate": (C.c_int, [_vp, _vp, C.POINTER(QleSynthCfg)]),
    "qle_synth_rmse": (C.c_int, [_vp, _vp, _pd]),
    "qle_synth_get_truth": (C.c_int, [_vp, _vp, _pd, _pd]),
    "qle_get_report": (C.c_int, [_vp, _pd, _pd, _pd, _pd]),
    "qle_get_node_report": (C.c_int, [_vp, C.POINTER(QleNodeReport)]),
    "qle_count_nonfinite": (C.c_int, [_vp, C.POINTER(_i64)]),
    "qle_synchronize": (C.c_int, [_vp]),
    "qle_timer_begin": (C.c_int, [_vp]),
    "qle_timer_end": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "qle_algorithmic_bytes": (_i64, [_vp, _i32]),
    "qle_get_policy": (C.c_int, [_vp, C.POINTER(QlePolicy)]),
    "qle_get_device_view": (C.c_int, [_vp, C.POINTER(QleDeviceView)]),
    "qle_inputs_get_device_view": (C.c_int, [_vp, _i64, C.POINTER(QleInputsView)]),
    "qle_launch_census_begin": (C.c_int, []),
    "qle_launch_census_end": (C.c_int, [C.c_char_p, _i64, C.POINTER(_i64)]),
}

def _bind(path, symbols, no_fallback):
    """CDLL(path) with every entry of `symbols`, name -> (restype, argtypes), typed; raises (never falls back) when the file is missing."""
    if not os.path.exists(path):
        raise ImportError(f"{path} not built: run `make -C quadrotor_landing_amd/csrc` (hipcc, gfx950). {no_fallback}")
    L = C.CDLL(path)
    for name, (res, args) in symbols.items():
        fn = getattr(L, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    return L


_lib = None


def lib():
    """Load libqle_ekf.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        _lib = _bind(LIB_PATH, SYMBOLS, "There is no CPU fallback for the EKF engine.")
    return _lib


def check(rc):
    if rc != QLE_OK:
        raise QleError(rc, lib().qle_last_error().decode())
    return rc


SIDE_LIBRARIES = {}   # stem -> SideLibrary, every one of the closed census (csrc/Makefile, SIDE) the package has made
OPEN_LIBRARIES = {}   # stem -> SideLibrary outside it (csrc/Makefile, SIDE_OPEN): a census of its own, `SideLibrary.launch_census`


class SideLibrary:
    """One of the libraries beside libqle_ekf.so (devio, gate, consistency, health, lookahead, sequence, score, bank, imm, adapt, stateio): where it is
    (`env` names the environment variable that overrides the in-tree path), what it exports (`symbols`, name -> (restype, argtypes)),
    `what` it is for (the error text when it is missing), the name of its `*_last_error`, and what has to be loaded in front of it.
    needs_tick_library: the library takes qle_params_derive from the tick library, which is loaded first so that it is the same copy
    the handle uses (QLE_LIB included); `after`: side libraries it links, loaded before either.  closed_census: the library is one of
    the Makefile's SIDE, whose kernels are the rows of the closed case table and which `side_launch_census` covers; False: it is one
    of SIDE_OPEN, registered in `OPEN_LIBRARIES`, with a case table of its own."""

    def __init__(self, stem, env, symbols, what, last_error, needs_tick_library=False, after=(), closed_census=True):
        self.stem, self.path = stem, os.environ.get(env) or os.path.join(_HERE, f"libqle_{stem}.so")
        self.symbols, self.what, self.last_error = symbols, what, last_error
        self.prefix = last_error[:-len("_last_error")]
        self.needs_tick_library, self.after = needs_tick_library, tuple(after)
        self._handle = None
        self.closed_census = closed_census
        (SIDE_LIBRARIES if closed_census else OPEN_LIBRARIES)[stem] = self

    def load(self):
        """The bound library, loaded on the first call; raises (never falls back) when it is missing."""
        if self._handle is None:
            for other in self.after:
                other.load()
            if self.needs_tick_library:
                lib()
            self._handle = _bind(self.path, self.symbols, f"There is no fallback for {self.what}.")
        return self._handle

    def check(self, rc):
        """rc of one of the library's entries (0, a count, or a negative QLE_ERR_*): raises `QleError` with the library's message for
        rc < 0 and returns rc otherwise."""
        if rc < 0:
            raise QleError(rc, getattr(self.load(), self.last_error)().decode())
        return rc

    @contextlib.contextmanager
    def launch_census(self):
        """Diagnostics: the distinct kernels this library launches inside the block, process-wide (`<prefix>_launch_census_begin` /
        `_end`).  Yields a list that is filled on exit with the kernels' demangled names, sorted by mangled name."""
        L = self.load()
        begin, end = getattr(L, self.prefix + "_launch_census_begin"), getattr(L, self.prefix + "_launch_census_end")
        names = []
        self.check(begin())
        try:
            yield names
        finally:
            names.extend(_census_names(end, self.check))


_cxa = None


def demangle(name):
    """Itanium C++ demangling through libstdc++'s __cxa_demangle (no external tool); a name it cannot parse is returned as is."""
    global _cxa
    if _cxa is None:
        cxx, libc = C.CDLL("libstdc++.so.6"), C.CDLL(None)
        cxx.__cxa_demangle.restype = C.c_void_p
        cxx.__cxa_demangle.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        libc.free.argtypes = [C.c_void_p]
        _cxa = (cxx.__cxa_demangle, libc.free)
    fn, free = _cxa
    status = C.c_int(0)
    p = fn(name.encode(), None, None, C.byref(status))
    if status.value != 0 or not p:
        return name
    try:
        return C.string_at(p).decode()
    finally:
        free(p)


@contextlib.contextmanager
def launch_census():
    """Diagnostics: the distinct kernels the library launches inside the block, process-wide (every handle, every host thread).
    Yields a list that is filled on exit with the kernels' demangled names, sorted by mangled name."""
    L = lib()
    names = []
    check(L.qle_launch_census_begin())
    try:
        yield names
    finally:
        names.extend(_census_names(L.qle_launch_census_end, check))


def _census_names(end, check_rc):
    """The list of a `*_launch_census_end` entry by its two-call size protocol, demangled."""
    need = _i64(0)
    check_rc(end(None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    check_rc(end(buf, need.value, C.byref(need)))
    return [demangle(n) for n in buf.value.decode().split("\n") if n]


@contextlib.contextmanager
def side_launch_census():
    """Diagnostics: `SideLibrary.launch_census` of every side library at once (each is loaded first).  Yields a dict that is filled on
    exit: {library stem: [demangled kernel names]}, a library that launched nothing with an empty list."""
    out = {}
    with contextlib.ExitStack() as stack:
        lists = {stem: stack.enter_context(side.launch_census()) for stem, side in sorted(SIDE_LIBRARIES.items())}
        try:
            yield out
        finally:
            stack.close()
            out.update(lists)
