"""ctypes binding of libmcconv.so — the C ABI declared in include/mcconv.h.

The product path has no CPU fallback: if the HIP library is missing or fails
to load, importing an engine raises.  (The CPU oracle lives under oracle/ and
is never imported from here.)
"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
# MCCONV_LIB: another build of the same library (A/B measurements of kernel variants); there is still no CPU path
LIB_PATH = os.environ.get("MCCONV_LIB") or os.path.join(HERE, "libmcconv.so")

MC_BLOCK = 256
MC_MAX_PREDELAY = 8192

# every symbol include/mcconv.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "mc_abi_version", "mc_last_error", "mc_default_config", "mc_default_params", "mc_create", "mc_destroy",
    "mc_reset", "mc_set_period", "mc_load_ir", "mc_load_ir_resampled", "mc_default_ir_shape", "mc_load_ir_shaped", "mc_ir_shape_info",
    "mc_default_ir_eq", "mc_load_ir_eq", "mc_ir_eq_response", "mc_default_ir_damp", "mc_load_ir_damped", "mc_ir_damp_info", "mc_ir_damp_response",
    "mc_default_ir_synth", "mc_synth_ir", "mc_ir_synth_info",
    "mc_default_sweep", "mc_sweep_generate", "mc_load_ir_sweep", "mc_ir_sweep_info",
    "mc_default_decay_query", "mc_ir_decay", "mc_default_floor_query", "mc_ir_floor", "mc_ir_tail_from_floor",
    "mc_default_density_query", "mc_ir_density", "mc_ir_tail_move_knee",
    "mc_default_iacc_query", "mc_ir_iacc", "mc_ir_tail_width_from_iacc",
    "mc_default_sti_query", "mc_ir_sti",
    "mc_default_response_query", "mc_ir_response", "mc_response_grid", "mc_response_smooth",
    "mc_default_ir_tail", "mc_load_ir_tail", "mc_load_ir_sweep_tail", "mc_ir_tail_info",
    "mc_default_ir_phase", "mc_ir_phase_plan", "mc_load_ir_phase", "mc_load_ir_sweep_phase", "mc_ir_phase_info",
    "mc_default_ir_filter", "mc_ir_filter_plan", "mc_load_ir_filter", "mc_load_ir_sweep_filter", "mc_ir_filter_info",
    "mc_default_ir_match", "mc_ir_match_plan", "mc_load_ir_match", "mc_load_ir_sweep_match", "mc_ir_match_info", "mc_ir_match_curve",
    "mc_default_ir_parts", "mc_ir_parts_plan", "mc_ir_parts_at", "mc_load_ir_parts", "mc_load_ir_sweep_parts", "mc_ir_parts_info",
    "mc_default_ir_room", "mc_synth_ir_room", "mc_ir_room_info", "mc_ir_room_plan",
    "mc_default_ir_room_mics", "mc_synth_ir_room_mics", "mc_ir_room_mics_plan", "mc_ir_room_mics_info",
    "mc_default_ir_room_bands", "mc_synth_ir_room_bands", "mc_ir_room_bands_plan", "mc_ir_room_bands_info",
    "mc_default_ir_room_head", "mc_synth_ir_room_head", "mc_ir_room_head_plan", "mc_ir_room_head_info",
    "mc_default_ir_plate", "mc_synth_ir_plate", "mc_ir_plate_plan", "mc_ir_plate_modes", "mc_ir_plate_info",
    "mc_default_ir_spring", "mc_synth_ir_spring", "mc_ir_spring_plan", "mc_ir_spring_response", "mc_ir_spring_info", "mc_num_irs", "mc_ir_info", "mc_set_params", "mc_get_params", "mc_handle_cc",
    "mc_process", "mc_process_batch", "mc_process_batch_device", "mc_partial_batch_device",
    "mc_finish_batch_device", "mc_finish_batch_slice_device", "mc_process_batch_slice_device", "mc_sync", "mc_fence", "mc_fence_older", "mc_set_stream", "mc_get_stream", "mc_avg_runtime_ms",
    "mc_enable_kernel_timing", "mc_get_kernel_stats", "mc_algorithmic_bytes_per_block", "mc_blocks_processed", "mc_preferred_batch",
    "mc_debug_read", "mc_host_alloc", "mc_host_free",
]


class McConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("n_ref", C.c_uint64),
        ("max_batch", C.c_uint32),
        ("max_partitions", C.c_uint32),
        ("compat", C.c_uint32),
        ("part_begin", C.c_uint32),
        ("part_end", C.c_uint32),
        ("stream_threshold", C.c_uint32),
        ("precision", C.c_uint32),
        ("period", C.c_uint32),
        ("pipeline", C.c_uint32),
        ("form", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class McCcValue(C.Structure):
    """Mirror of Convolution::CC::value (reference src/conv.h:38-49)."""

    _fields_ = [
        ("select", C.c_uint64),
        ("predelay", C.c_uint64),
        ("speed", C.c_uint64),
        ("vsteps", C.c_uint64),
        ("dry", C.c_float),
        ("wet", C.c_float),
        ("panDry", C.c_float),
        ("panWet", C.c_float),
        ("level", C.c_float),
    ]


MC_SHAPE_REVERSE = 1
MC_NORM_NONE, MC_NORM_PEAK, MC_NORM_ENERGY = 0, 1, 2


class McIrShape(C.Structure):
    """mc_ir_shape: what mc_load_ir_shaped does to an IR before it is truncated and transformed."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("flags", C.c_uint32),
        ("start", C.c_uint64),
        ("length", C.c_uint64),
        ("decay_t60", C.c_uint64),
        ("fade_out", C.c_uint64),
        ("trim_db", C.c_float),
        ("pre_roll", C.c_uint32),
        ("normalize", C.c_uint32),
        ("target", C.c_float),
    ]


MC_EQ_MAX_BANDS = 8
MC_EQ_OFF, MC_EQ_LOWCUT, MC_EQ_HIGHCUT, MC_EQ_LOWSHELF, MC_EQ_HIGHSHELF, MC_EQ_PEAK = range(6)


class McEqBand(C.Structure):
    """mc_eq_band: one biquad of the EQ mc_load_ir_eq applies to an IR."""

    _fields_ = [
        ("kind", C.c_uint32),
        ("freq_hz", C.c_float),
        ("gain_db", C.c_float),
        ("q", C.c_float),
    ]


class McIrEq(C.Structure):
    """mc_ir_eq: up to MC_EQ_MAX_BANDS bands, applied in index order."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("reserved", C.c_uint32),
        ("band", McEqBand * MC_EQ_MAX_BANDS),
    ]


MC_DAMP_MAX_XOVERS = 3


class McIrDamp(C.Structure):
    """mc_ir_damp: a further decay per frequency band, applied by mc_load_ir_damped between the fade and the EQ."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_xovers", C.c_uint32),
        ("xover_hz", C.c_float * MC_DAMP_MAX_XOVERS),
        ("reserved", C.c_uint32),
        ("decay_t60", C.c_uint64 * (MC_DAMP_MAX_XOVERS + 1)),
        ("origin", C.c_uint64),
    ]


MC_SYNTH_MAX_EARLY = 64


class McIrSynth(C.Structure):
    """mc_ir_synth: the IR mc_synth_ir generates on the device from a seed."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_early", C.c_uint32),
        ("seed", C.c_uint64),
        ("frames", C.c_uint64),
        ("late_start", C.c_uint64),
        ("t60", C.c_uint64),
        ("build_up", C.c_uint32),
        ("late_gain", C.c_float),
        ("direct", C.c_float),
        ("early_gain", C.c_float),
        ("width", C.c_float),
        ("rate", C.c_uint32),
        ("early_first", C.c_uint64),
        ("early_last", C.c_uint64),
    ]


class McSweep(C.Structure):
    """mc_sweep: the exponential sine sweep whose recording mc_load_ir_sweep deconvolves."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("rate", C.c_uint32),
        ("frames", C.c_uint64),
        ("f1_hz", C.c_float),
        ("f2_hz", C.c_float),
        ("amplitude", C.c_float),
        ("fade_in", C.c_uint32),
        ("fade_out", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


MC_DECAY_MAX_BANDS = 10
MC_DECAY_MAX_CURVE = 1024


class McDecayQuery(C.Structure):
    """mc_decay_query: what mc_ir_decay measures of a loaded IR."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("rate", C.c_uint32),
        ("n_bands", C.c_uint32),
        ("curve_points", C.c_uint32),
        ("centre_hz", C.c_float * MC_DECAY_MAX_BANDS),
        ("q", C.c_float),
        ("onset_db", C.c_float),
        ("end", C.c_uint64),
    ]


MC_FLOOR_MAX_XOVERS = 3


class McFloorQuery(C.Structure):
    """mc_floor_query: how mc_ir_floor searches a loaded IR for its noise floor."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("rate", C.c_uint32),
        ("n_xovers", C.c_uint32),
        ("window", C.c_uint32),
        ("xover_hz", C.c_float * MC_FLOOR_MAX_XOVERS),
        ("onset_db", C.c_float),
        ("end", C.c_uint64),
        ("tail_fraction", C.c_float),
        ("margin_db", C.c_float),
        ("span_db", C.c_float),
        ("per_decade", C.c_uint32),
        ("rounds", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class McDensityQuery(C.Structure):
    """mc_density_query: how mc_ir_density measures a loaded IR's echo density."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("rate", C.c_uint32),
        ("half", C.c_uint32),
        ("hop", C.c_uint32),
        ("onset_db", C.c_float),
        ("threshold", C.c_float),
        ("end", C.c_uint64),
        ("decay_t60", C.c_uint64),
        ("reserved", C.c_uint32 * 2),
    ]


MC_IACC_MAX_LAG = 1024


class McIaccQuery(C.Structure):
    """mc_iacc_query: how mc_ir_iacc measures a loaded IR's interaural cross-correlation."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("rate", C.c_uint32),
        ("n_bands", C.c_uint32),
        ("max_lag", C.c_uint32),
        ("centre_hz", C.c_float * MC_DECAY_MAX_BANDS),
        ("q", C.c_float),
        ("onset_db", C.c_float),
        ("end", C.c_uint64),
        ("split", C.c_uint64),
        ("reserved", C.c_uint32 * 2),
    ]


MC_STI_MAX_BANDS = 7
MC_STI_MAX_MOD = 16
MC_STI_SNR = 1


class McStiQuery(C.Structure):
    """mc_sti_query: how mc_ir_sti measures a loaded IR's speech transmission index."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("rate", C.c_uint32),
        ("n_bands", C.c_uint32),
        ("n_mod", C.c_uint32),
        ("flags", C.c_uint32),
        ("centre_hz", C.c_float * MC_STI_MAX_BANDS),
        ("alpha", C.c_double * MC_STI_MAX_BANDS),
        ("beta", C.c_double * (MC_STI_MAX_BANDS - 1)),
        ("snr_db", C.c_float * MC_STI_MAX_BANDS),
        ("mod_hz", C.c_float * MC_STI_MAX_MOD),
        ("q", C.c_float),
        ("onset_db", C.c_float),
        ("end", C.c_uint64),
        ("reserved", C.c_uint32 * 2),
    ]


MC_RSP_MAX_FREQ = 1024
MC_RSP_MAX_WIN = 64


class McResponseWindow(C.Structure):
    """mc_response_window: the taps of one window of mc_ir_response, counted from the origin, and its raised-cosine edges."""

    _fields_ = [("first", C.c_uint64), ("count", C.c_uint64), ("rise", C.c_uint32), ("fall", C.c_uint32)]


class McResponseQuery(C.Structure):
    """mc_response_query: how mc_ir_response measures a loaded IR's frequency response."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("rate", C.c_uint32),
        ("n_freq", C.c_uint32),
        ("n_win", C.c_uint32),
        ("flags", C.c_uint32),
        ("onset_db", C.c_float),
        ("end", C.c_uint64),
        ("reserved", C.c_uint32 * 2),
    ]


MC_TAIL_OFF, MC_TAIL_CUT, MC_TAIL_EXTEND = 0, 1, 2
MC_TAIL_LEFT_ALONE = (1 << 64) - 1  # a knee that leaves its band alone


class McIrTail(C.Structure):
    """mc_ir_tail: the tail step of mc_load_ir_tail and mc_load_ir_sweep_tail, a knee per frequency band."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("mode", C.c_uint32),
        ("n_xovers", C.c_uint32),
        ("xover_hz", C.c_float * 3),
        ("fade", C.c_uint32),
        ("width", C.c_float),
        ("seed", C.c_uint64),
        ("length", C.c_uint64),
        ("knee", C.c_uint64 * 4),
        ("t60", C.c_uint64 * 4),
        ("level_db", (C.c_float * 2) * 4),
    ]


MC_PHASE_OFF, MC_PHASE_MINIMUM = 0, 1


class McIrPhase(C.Structure):
    """mc_ir_phase: the phase step of mc_load_ir_phase and mc_load_ir_sweep_phase."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("mode", C.c_uint32),
        ("floor_db", C.c_float),
        ("over_log2", C.c_uint32),
    ]


MC_FILTER_OFF, MC_FILTER_CONVOLVE, MC_FILTER_DECONVOLVE = 0, 1, 2
MC_FILTER_STEREO, MC_FILTER_LEFT, MC_FILTER_MID = 0, 1, 2


class McIrFilter(C.Structure):
    """mc_ir_filter: the filter step of mc_load_ir_filter and mc_load_ir_sweep_filter."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("op", C.c_uint32),
        ("channels", C.c_uint32),
        ("rate", C.c_uint32),
        ("reg_db", C.c_float),
        ("reserved", C.c_uint32),
        ("frames_out", C.c_uint64),
    ]


MC_MATCH_OFF, MC_MATCH_TARGET, MC_MATCH_FLAT = 0, 1, 2
MC_MATCH_MINIMUM, MC_MATCH_LINEAR = 0, 1
MC_MATCH_MAX_POINTS = 1024


class McIrMatch(C.Structure):
    """mc_ir_match: the match step of mc_load_ir_match and mc_load_ir_sweep_match."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("mode", C.c_uint32),
        ("phase", C.c_uint32),
        ("link", C.c_uint32),
        ("rate", C.c_uint32),
        ("per_octave", C.c_uint32),
        ("lo_hz", C.c_double),
        ("hi_hz", C.c_double),
        ("octaves", C.c_double),
        ("amount", C.c_float),
        ("boost_db", C.c_float),
        ("cut_db", C.c_float),
        ("floor_db", C.c_float),
        ("tilt_db", C.c_float),
        ("delay", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


MC_PARTS_OFF, MC_PARTS_ON = 0, 1


class McIrParts(C.Structure):
    """mc_ir_parts: the parts step of mc_load_ir_parts and mc_load_ir_sweep_parts."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("mode", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved0", C.c_uint32),
        ("direct_end", C.c_uint64),
        ("early_end", C.c_uint64),
        ("xfade", C.c_uint32 * 2),
        ("delay", C.c_int32 * 3),
        ("gain_db", C.c_float * 3),
        ("width", C.c_float * 3),
        ("balance", C.c_float * 3),
        ("frames_out", C.c_uint64),
        ("reserved", C.c_uint32 * 2),
    ]


MC_ROOM_MAX_ORDER = 32


class McIrRoom(C.Structure):
    """mc_ir_room: the rectangular room whose reflections mc_synth_ir_room adds to a synthesised IR."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("order", C.c_uint32),
        ("size_m", C.c_float * 3),
        ("source_m", C.c_float * 3),
        ("receiver_m", C.c_float * 3),
        ("beta", C.c_float * 6),
        ("spacing_m", C.c_float),
        ("axis", C.c_uint32),
        ("speed", C.c_float),
        ("gain", C.c_float),
        ("reserved", C.c_uint32),
        ("last", C.c_uint64),
    ]


class McIrRoomMics(C.Structure):
    """mc_ir_room_mics: the patterns and aims of the two receivers and of the source in the room of mc_synth_ir_room_mics."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("flags", C.c_uint32),
        ("mic_pattern", C.c_float * 2),
        ("mic_az_deg", C.c_float * 2),
        ("mic_el_deg", C.c_float * 2),
        ("src_pattern", C.c_float),
        ("src_az_deg", C.c_float),
        ("src_el_deg", C.c_float),
        ("reserved", C.c_uint32),
    ]


class McIrRoomBands(C.Structure):
    """mc_ir_room_bands: the walls and the air of the room of mc_synth_ir_room_bands per frequency band."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_xovers", C.c_uint32),
        ("xover_hz", C.c_float * 3),
        ("beta", (C.c_float * 6) * 4),
        ("air_db_per_m", C.c_float * 4),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class McIrRoomHead(C.Structure):
    """mc_ir_room_head: the rigid-sphere listener that mc_synth_ir_room_head puts in the room in place of the receiver pair."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("flags", C.c_uint32),
        ("radius_m", C.c_float),
        ("facing_az_deg", C.c_float),
        ("ear_deg", C.c_float),
        ("shadow", C.c_float),
        ("reserved", C.c_uint32 * 2),
    ]


MC_PLATE_MAX_MODES = 1 << 18
MC_PLATE_GROUP = 32
MC_PLATE_SLAB = 256
MC_PLATE_MAX_PAIRS = 1 << 36


class McIrPlate(C.Structure):
    """mc_ir_plate: the plate whose modes mc_synth_ir_plate adds to a synthesised IR."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("size_m", C.c_float * 2),
        ("thickness_mm", C.c_float),
        ("young_gpa", C.c_float),
        ("density", C.c_float),
        ("poisson", C.c_float),
        ("driver_m", C.c_float * 2),
        ("pickup_m", (C.c_float * 2) * 2),
        ("low_hz", C.c_float),
        ("high_hz", C.c_float),
        ("t60_s", C.c_float * 2),
        ("damp_hz", C.c_float),
        ("gain", C.c_float),
        ("reserved", C.c_uint32),
        ("last", C.c_uint64),
    ]


MC_SPRING_MAX = 3
MC_SPRING_MAX_STRETCH = 64
MC_SPRING_RADIUS = 1e8
MC_SPRING_MAX_LOG2 = 22


class McIrSpring(C.Structure):
    """mc_ir_spring: the spring tank whose response mc_synth_ir_spring adds to a synthesised IR."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("sections", C.c_uint32),
        ("transition_hz", C.c_float),
        ("dispersion", C.c_float),
        ("delay_ms", C.c_float * 3),
        ("t60_s", C.c_float),
        ("damping", C.c_float),
        ("lowpass_order", C.c_uint32),
        ("high_gain", C.c_float),
        ("high_sections", C.c_uint32),
        ("high_dispersion", C.c_float),
        ("high_delay", C.c_float),
        ("high_t60_s", C.c_float),
        ("stereo", C.c_float),
        ("gain", C.c_float),
        ("log2_points", C.c_uint32),
        ("last", C.c_uint64),
    ]


class McKernelStats(C.Structure):
    _fields_ = [
        ("launches", C.c_uint64),
        ("blocks", C.c_uint64),
        ("total_ms", C.c_double),
        ("last_ms", C.c_double),
        ("resident", C.c_uint32),
        ("partitions", C.c_uint32),
        ("fast_levels", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


_lib = None


def load():
    """Load libmcconv.so; raise (never fall back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m cuda_audio_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own
    # libamdhip64/libhsa-runtime64.  If libmcconv.so is loaded first it binds to
    # /opt/rocm's copies and a later `import torch` finds "No HIP GPUs"; loaded
    # after torch it binds (by soname) to torch's runtime, and stream handles
    # and device pointers interoperate.  So when torch is installed, load it
    # first.  Hosts without Python/torch (cuda_audio_amd/host) use /opt/rocm's.
    if "torch" not in sys.modules and os.environ.get("MCCONV_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    vp, fp, u64 = C.c_void_p, C.POINTER(C.c_float), C.c_uint64
    L.mc_abi_version.restype = C.c_uint32
    L.mc_last_error.restype = C.c_char_p
    L.mc_default_config.argtypes = [C.POINTER(McConfig)]
    L.mc_default_params.argtypes = [C.POINTER(McCcValue)]
    L.mc_create.argtypes = [C.POINTER(McConfig), C.POINTER(vp)]
    L.mc_destroy.argtypes = [vp]
    L.mc_destroy.restype = None
    L.mc_reset.argtypes = [vp]
    L.mc_set_period.argtypes = [vp, C.c_uint32]
    L.mc_load_ir.argtypes = [vp, u64, fp, u64, u64]
    L.mc_load_ir_resampled.argtypes = [vp, u64, fp, u64, u64, C.c_uint32, C.c_uint32]
    L.mc_default_ir_shape.argtypes = [C.POINTER(McIrShape)]
    L.mc_default_ir_shape.restype = None
    L.mc_load_ir_shaped.argtypes = [vp, u64, fp, u64, u64, C.c_uint32, C.c_uint32, C.POINTER(McIrShape)]
    L.mc_ir_shape_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_default_ir_eq.argtypes = [C.POINTER(McIrEq)]
    L.mc_default_ir_eq.restype = None
    L.mc_load_ir_eq.argtypes = [vp, u64, fp, u64, u64, C.c_uint32, C.c_uint32, C.POINTER(McIrShape), C.POINTER(McIrEq)]
    L.mc_ir_eq_response.argtypes = [C.POINTER(McIrEq), C.c_uint32, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double)]
    L.mc_default_ir_damp.argtypes = [C.POINTER(McIrDamp)]
    L.mc_default_ir_damp.restype = None
    L.mc_load_ir_damped.argtypes = [vp, u64, fp, u64, u64, C.c_uint32, C.c_uint32, C.POINTER(McIrShape), C.POINTER(McIrEq), C.POINTER(McIrDamp)]
    L.mc_ir_damp_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_ir_damp_response.argtypes = [C.POINTER(McIrDamp), C.c_uint32, u64, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double)]
    L.mc_default_ir_synth.argtypes = [C.POINTER(McIrSynth)]
    L.mc_default_ir_synth.restype = None
    L.mc_synth_ir.argtypes = [vp, u64, u64, C.POINTER(McIrSynth), C.POINTER(McIrShape), C.POINTER(McIrEq), C.POINTER(McIrDamp)]
    L.mc_ir_synth_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_default_sweep.argtypes = [C.POINTER(McSweep)]
    L.mc_default_sweep.restype = None
    L.mc_sweep_generate.argtypes = [C.POINTER(McSweep), fp, u64, u64]
    L.mc_load_ir_sweep.argtypes = [vp, u64, fp, u64, u64, C.POINTER(McSweep), C.c_int64, u64, C.POINTER(McIrShape), C.POINTER(McIrEq), C.POINTER(McIrDamp)]
    L.mc_ir_sweep_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_default_decay_query.argtypes = [C.POINTER(McDecayQuery)]
    L.mc_default_decay_query.restype = None
    L.mc_ir_decay.argtypes = [vp, u64, C.POINTER(McDecayQuery), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(u64)]
    L.mc_default_floor_query.argtypes = [C.POINTER(McFloorQuery)]
    L.mc_default_floor_query.restype = None
    L.mc_ir_floor.argtypes = [vp, u64, C.POINTER(McFloorQuery), C.POINTER(C.c_double), C.POINTER(u64)]
    L.mc_ir_tail_from_floor.argtypes = [C.POINTER(McFloorQuery), C.POINTER(C.c_double), C.POINTER(u64), u64, C.POINTER(McIrTail)]
    L.mc_default_density_query.argtypes = [C.POINTER(McDensityQuery)]
    L.mc_default_density_query.restype = None
    L.mc_ir_density.argtypes = [vp, u64, C.POINTER(McDensityQuery), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(u64)]
    L.mc_ir_tail_move_knee.argtypes = [C.POINTER(McIrTail), C.c_uint32, u64]
    L.mc_default_iacc_query.argtypes = [C.POINTER(McIaccQuery)]
    L.mc_default_iacc_query.restype = None
    L.mc_ir_iacc.argtypes = [vp, u64, C.POINTER(McIaccQuery), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(u64)]
    L.mc_ir_tail_width_from_iacc.argtypes = [C.POINTER(McIrTail), C.c_double]
    L.mc_default_sti_query.argtypes = [C.POINTER(McStiQuery)]
    L.mc_default_sti_query.restype = None
    L.mc_ir_sti.argtypes = [vp, u64, C.POINTER(McStiQuery), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(u64)]
    L.mc_default_response_query.argtypes = [C.POINTER(McResponseQuery)]
    L.mc_default_response_query.restype = None
    L.mc_ir_response.argtypes = [vp, u64, C.POINTER(McResponseQuery), fp, C.POINTER(McResponseWindow), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                 C.POINTER(u64), C.POINTER(u64)]
    L.mc_response_grid.argtypes = [C.c_double, C.c_double, C.c_uint32, fp, C.c_uint32]
    L.mc_response_smooth.argtypes = [fp, C.POINTER(C.c_double), C.c_uint32, C.c_double, C.POINTER(C.c_double)]
    L.mc_default_ir_tail.argtypes = [C.POINTER(McIrTail)]
    L.mc_default_ir_tail.restype = None
    L.mc_load_ir_tail.argtypes = [vp, u64, fp, u64, u64, C.c_uint32, C.c_uint32, C.POINTER(McIrShape), C.POINTER(McIrEq), C.POINTER(McIrDamp),
                                  C.POINTER(McIrTail)]
    L.mc_load_ir_sweep_tail.argtypes = [vp, u64, fp, u64, u64, C.POINTER(McSweep), C.c_int64, u64, C.POINTER(McIrShape), C.POINTER(McIrEq),
                                        C.POINTER(McIrDamp), C.POINTER(McIrTail)]
    L.mc_ir_tail_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_default_ir_phase.argtypes = [C.POINTER(McIrPhase)]
    L.mc_default_ir_phase.restype = None
    L.mc_ir_phase_plan.argtypes = [C.POINTER(McIrPhase), u64, C.POINTER(C.c_double)]
    L.mc_load_ir_phase.argtypes = L.mc_load_ir_tail.argtypes + [C.POINTER(McIrPhase)]
    L.mc_load_ir_sweep_phase.argtypes = L.mc_load_ir_sweep_tail.argtypes + [C.POINTER(McIrPhase)]
    L.mc_ir_phase_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_default_ir_filter.argtypes = [C.POINTER(McIrFilter)]
    L.mc_default_ir_filter.restype = None
    L.mc_ir_filter_plan.argtypes = [C.POINTER(McIrFilter), u64, u64, C.POINTER(C.c_double)]
    L.mc_load_ir_filter.argtypes = L.mc_load_ir_phase.argtypes + [C.POINTER(McIrFilter), fp, u64]
    L.mc_load_ir_sweep_filter.argtypes = L.mc_load_ir_sweep_phase.argtypes + [C.POINTER(McIrFilter), fp, u64]
    L.mc_ir_filter_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_default_ir_match.argtypes = [C.POINTER(McIrMatch)]
    L.mc_default_ir_match.restype = None
    L.mc_ir_match_plan.argtypes = [C.POINTER(McIrMatch), u64, u64, C.c_uint32, C.POINTER(C.c_double)]
    L.mc_load_ir_match.argtypes = L.mc_load_ir_filter.argtypes + [C.POINTER(McIrMatch), fp, u64]
    L.mc_load_ir_sweep_match.argtypes = L.mc_load_ir_sweep_filter.argtypes + [C.POINTER(McIrMatch), fp, u64]
    L.mc_ir_match_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_ir_match_curve.argtypes = [vp, u64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32]
    L.mc_default_ir_parts.argtypes = [C.POINTER(McIrParts)]
    L.mc_default_ir_parts.restype = None
    L.mc_ir_parts_plan.argtypes = [C.POINTER(McIrParts), u64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mc_ir_parts_at.argtypes = [C.POINTER(McIrParts), u64, u64, u64]
    L.mc_load_ir_parts.argtypes = L.mc_load_ir_match.argtypes + [C.POINTER(McIrParts)]
    L.mc_load_ir_sweep_parts.argtypes = L.mc_load_ir_sweep_match.argtypes + [C.POINTER(McIrParts)]
    L.mc_ir_parts_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_default_ir_room.argtypes = [C.POINTER(McIrRoom)]
    L.mc_default_ir_room.restype = None
    L.mc_synth_ir_room.argtypes = [vp, u64, u64, C.POINTER(McIrSynth), C.POINTER(McIrRoom), C.POINTER(McIrShape), C.POINTER(McIrEq), C.POINTER(McIrDamp),
                                   C.POINTER(McIrTail)]
    L.mc_ir_room_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_ir_room_plan.argtypes = [C.POINTER(McIrRoom), C.c_uint32, u64, C.POINTER(C.c_double)]
    L.mc_default_ir_room_mics.argtypes = [C.POINTER(McIrRoomMics)]
    L.mc_default_ir_room_mics.restype = None
    L.mc_synth_ir_room_mics.argtypes = [vp, u64, u64, C.POINTER(McIrSynth), C.POINTER(McIrRoom), C.POINTER(McIrRoomMics), C.POINTER(McIrShape),
                                        C.POINTER(McIrEq), C.POINTER(McIrDamp), C.POINTER(McIrTail)]
    L.mc_ir_room_mics_plan.argtypes = [C.POINTER(McIrRoom), C.POINTER(McIrRoomMics), C.c_uint32, u64, C.POINTER(C.c_double)]
    L.mc_ir_room_mics_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_default_ir_room_bands.argtypes = [C.POINTER(McIrRoomBands)]
    L.mc_default_ir_room_bands.restype = None
    L.mc_synth_ir_room_bands.argtypes = [vp, u64, u64, C.POINTER(McIrSynth), C.POINTER(McIrRoom), C.POINTER(McIrRoomMics), C.POINTER(McIrRoomBands),
                                         C.POINTER(McIrShape), C.POINTER(McIrEq), C.POINTER(McIrDamp), C.POINTER(McIrTail)]
    L.mc_ir_room_bands_plan.argtypes = [C.POINTER(McIrRoom), C.POINTER(McIrRoomBands), C.c_uint32, u64, C.POINTER(C.c_double)]
    L.mc_ir_room_bands_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_default_ir_room_head.argtypes = [C.POINTER(McIrRoomHead)]
    L.mc_default_ir_room_head.restype = None
    L.mc_synth_ir_room_head.argtypes = [vp, u64, u64, C.POINTER(McIrSynth), C.POINTER(McIrRoom), C.POINTER(McIrRoomMics), C.POINTER(McIrRoomBands),
                                        C.POINTER(McIrRoomHead), C.POINTER(McIrShape), C.POINTER(McIrEq), C.POINTER(McIrDamp), C.POINTER(McIrTail)]
    L.mc_ir_room_head_plan.argtypes = [C.POINTER(McIrRoom), C.POINTER(McIrRoomHead), C.c_uint32, u64, C.POINTER(C.c_double)]
    L.mc_ir_room_head_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_default_ir_plate.argtypes = [C.POINTER(McIrPlate)]
    L.mc_default_ir_plate.restype = None
    L.mc_synth_ir_plate.argtypes = [vp, u64, u64, C.POINTER(McIrSynth), C.POINTER(McIrPlate), C.POINTER(McIrShape), C.POINTER(McIrEq), C.POINTER(McIrDamp),
                                    C.POINTER(McIrTail)]
    L.mc_ir_plate_plan.argtypes = [C.POINTER(McIrPlate), C.c_uint32, u64, C.POINTER(C.c_double)]
    L.mc_ir_plate_modes.argtypes = [C.POINTER(McIrPlate), C.c_uint32, u64, u64, C.POINTER(C.c_double)]
    L.mc_ir_plate_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_default_ir_spring.argtypes = [C.POINTER(McIrSpring)]
    L.mc_default_ir_spring.restype = None
    L.mc_synth_ir_spring.argtypes = [vp, u64, u64, C.POINTER(McIrSynth), C.POINTER(McIrSpring), C.POINTER(McIrShape), C.POINTER(McIrEq), C.POINTER(McIrDamp),
                                     C.POINTER(McIrTail)]
    L.mc_ir_spring_plan.argtypes = [C.POINTER(McIrSpring), C.c_uint32, u64, C.POINTER(C.c_double)]
    L.mc_ir_spring_response.argtypes = [C.POINTER(McIrSpring), C.c_uint32, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double)]
    L.mc_ir_spring_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_num_irs.argtypes = [vp]
    L.mc_ir_info.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.mc_set_params.argtypes = [vp, C.c_int, C.POINTER(McCcValue)]
    L.mc_get_params.argtypes = [vp, C.c_int, C.POINTER(McCcValue)]
    L.mc_handle_cc.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8), C.c_uint8, C.c_int]
    L.mc_process.argtypes = [vp, fp, fp, fp, fp, u64]
    L.mc_process_batch.argtypes = [vp, fp, fp, fp, fp, u64]
    L.mc_process_batch_device.argtypes = [vp, vp, vp, vp, vp, u64]
    L.mc_process_batch_slice_device.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64]
    L.mc_partial_batch_device.argtypes = [vp, vp, vp, vp, u64]
    L.mc_finish_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, u64]
    L.mc_finish_batch_slice_device.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, u64]
    L.mc_sync.argtypes = [vp]
    L.mc_fence.argtypes = [vp]
    L.mc_fence_older.argtypes = [vp]
    L.mc_set_stream.argtypes = [vp, vp]
    L.mc_get_stream.argtypes = [vp]
    L.mc_get_stream.restype = vp
    L.mc_avg_runtime_ms.argtypes = [vp]
    L.mc_avg_runtime_ms.restype = C.c_double
    L.mc_enable_kernel_timing.argtypes = [vp, C.c_int]
    L.mc_get_kernel_stats.argtypes = [vp, C.POINTER(McKernelStats), C.c_int]
    L.mc_algorithmic_bytes_per_block.argtypes = [vp]
    L.mc_algorithmic_bytes_per_block.restype = u64
    L.mc_blocks_processed.argtypes = [vp]
    L.mc_blocks_processed.restype = u64
    L.mc_preferred_batch.argtypes = [vp, u64]
    L.mc_preferred_batch.restype = u64
    L.mc_debug_read.argtypes = [vp, C.c_int, u64, vp, u64, u64, C.POINTER(u64)]
    L.mc_host_alloc.argtypes = [C.c_size_t]
    L.mc_host_alloc.restype = vp
    L.mc_host_free.argtypes = [vp]
    L.mc_host_free.restype = None
    _lib = L
    return L


class McError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mcconv error {code}: {msg}")
        self.code = code


def check(rc):
    if rc != 0:
        raise McError(rc, load().mc_last_error().decode("utf-8", "replace"))
