"""ctypes binding of the framework's C-ABI (include/xg_sched.h, include/xg.h).

Python is only the harness here (bench.py, tests): every byte of the exchange
is moved by lib/libxg.so (HIP kernels + RCCL) and every schedule comes from
lib/libxghost.so.  There is no fallback: if a library is missing, loading
fails with an error that says how to build it.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.environ.get("XG_LIBDIR") or os.path.join(HERE, "lib")   # XG_LIBDIR: e.g. a sanitizer build of libxghost


class XGError(RuntimeError):
    pass


class Timer(C.Structure):
    """Timer of the reference (mpi_test.c:25-31)."""
    _fields_ = [("post_request_time", C.c_double), ("send_wait_all_time", C.c_double),
                ("recv_wait_all_time", C.c_double), ("barrier_time", C.c_double),
                ("total_time", C.c_double)]

    def as_tuple(self):
        return (self.post_request_time, self.send_wait_all_time, self.recv_wait_all_time,
                self.barrier_time, self.total_time)


NBUF = 5   # XG_NBUF


class Msg(C.Structure):
    _fields_ = [("src", C.c_int32), ("sseg", C.c_int32), ("dst", C.c_int32), ("dslot", C.c_int32),
                ("len", C.c_int64), ("step", C.c_int32), ("flags", C.c_int32),
                ("sbuf", C.c_int32), ("dbuf", C.c_int32), ("soff", C.c_int64), ("doff", C.c_int64)]


class Copy(C.Structure):
    _fields_ = [("src_off", C.c_int64), ("dst_off", C.c_int64), ("len", C.c_int64),
                ("src_buf", C.c_int32), ("dst_buf", C.c_int32)]


class P2P(C.Structure):
    _fields_ = [("off", C.c_int64), ("len", C.c_int64), ("peer", C.c_int32), ("buf", C.c_int32),
                ("is_send", C.c_int32), ("group", C.c_int32)]


class StepPlan(C.Structure):
    _fields_ = [("pre_begin", C.c_int32), ("pre_count", C.c_int32), ("p2p_begin", C.c_int32),
                ("p2p_count", C.c_int32), ("post_begin", C.c_int32), ("post_count", C.c_int32),
                ("sync_after", C.c_int32), ("stage_count", C.c_int32), ("posts", C.c_int32)]


class DevPlan(C.Structure):
    _fields_ = [("gpu", C.c_int32), ("ngpus", C.c_int32), ("nsteps", C.c_int32), ("flags", C.c_int32),
                ("region_bytes", C.c_int64 * NBUF), ("ncopy", C.c_int32), ("np2p", C.c_int32),
                ("copies", C.POINTER(Copy)), ("p2p", C.POINTER(P2P)), ("steps", C.POINTER(StepPlan)),
                ("local_bytes", C.c_int64), ("remote_send_bytes", C.c_int64),
                ("remote_recv_bytes", C.c_int64)]


class Call(C.Structure):
    """xg_call: one RCCL call of a step (XG_CALL_SEND / RECV / BARRIER)."""
    _fields_ = [("kind", C.c_int32), ("peer", C.c_int32), ("buf", C.c_int32), ("pad", C.c_int32),
                ("off", C.c_int64), ("len", C.c_int64)]


class CallPair(C.Structure):
    _fields_ = [("step", C.c_int32), ("src", C.c_int32), ("dst", C.c_int32), ("send_call", C.c_int32),
                ("recv_call", C.c_int32), ("group", C.c_int32), ("len", C.c_int64)]


CALL_SEND, CALL_RECV, CALL_BARRIER = 1, 2, 3


class SoloShape(C.Structure):
    _fields_ = [("rails", C.c_int32), ("npieces", C.c_int32), ("nrows", C.c_int32), ("nmeta", C.c_int32)]


ENG_LINES = 16                          # XG_ENG_LINES


class EngSoloState(C.Structure):
    """xg_eng_solo_state: the solo engine's counter words after some armed launches"""
    _fields_ = [("arrive", C.c_uint32), ("rails", C.c_uint32), ("go", C.c_uint32), ("fin", C.c_uint32 * ENG_LINES)]


class Span(C.Structure):
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("len", C.c_uint64)]


class SegRun(C.Structure):
    _fields_ = [("rank", C.c_int32), ("seed0", C.c_int32), ("off", C.c_int64), ("nsegs", C.c_int32),
                ("pad", C.c_int32)]


class Slot(C.Structure):
    _fields_ = [("src", C.c_int32), ("seed", C.c_int32), ("dst", C.c_int32), ("pad", C.c_int32),
                ("off", C.c_int64)]


class Delivery(C.Structure):
    """xg_delivery: receive slot `slot` of rank dst (recv_off in dst_gpu's RECV) must equal the
    segment at send_off of src_gpu's SEND."""
    _fields_ = [("src", C.c_int32), ("seed", C.c_int32), ("dst", C.c_int32), ("slot", C.c_int32),
                ("src_gpu", C.c_int32), ("dst_gpu", C.c_int32), ("send_off", C.c_int64), ("recv_off", C.c_int64)]


class BufSpan(C.Structure):
    """xg_bufspan: len bytes at off of region buf"""
    _fields_ = [("buf", C.c_int32), ("pad", C.c_int32), ("off", C.c_int64), ("len", C.c_int64)]


class Ext(C.Structure):
    """xg_ext: len bytes of pair (rank, aggregator index agg) at byte off of aggregator agg's domain"""
    _fields_ = [("rank", C.c_int32), ("agg", C.c_int32), ("off", C.c_int64), ("len", C.c_int64)]


class Vec(C.Structure):
    """xg_vec: count blocks of len bytes of pair (rank, aggregator index agg), block j at byte
    off + j * stride of aggregator agg's domain"""
    _fields_ = [("rank", C.c_int32), ("agg", C.c_int32), ("off", C.c_int64), ("len", C.c_int64),
                ("stride", C.c_int64), ("count", C.c_int64)]


class VRow(C.Structure):
    """xg_vrow: one table row of a strided placement -- count blocks of len bytes, block j from
    src_off + j * src_step of region src_buf to dst_off + j * dst_step of region dst_buf"""
    _fields_ = [("src_buf", C.c_int32), ("dst_buf", C.c_int32), ("src_off", C.c_int64), ("dst_off", C.c_int64),
                ("src_step", C.c_int64), ("dst_step", C.c_int64), ("len", C.c_int64), ("count", C.c_int64)]


class VecAt(C.Structure):
    """xg_vec_at"""
    _fields_ = [("src_off", C.c_int64), ("dst_off", C.c_int64), ("n", C.c_int64)]


class LaunchFacts(C.Structure):
    """xg_launch_facts: what one copy launch is"""
    _fields_ = [("bytes", C.c_int64), ("npos", C.c_int64), ("bits", C.c_uint64), ("uniform_len", C.c_int64),
                ("lens", C.POINTER(C.c_int64)), ("nlens", C.c_int32), ("dp_flags", C.c_int32), ("cross", C.c_int32),
                ("may_small", C.c_int32), ("nt_cut", C.c_int32), ("nt_run", C.c_int32)]


class CopyRules(C.Structure):
    """xg_copy_rules: the context's knobs; the defaults are the runtime's on a 256-CU device"""
    _fields_ = [("chunk", C.c_int64), ("wave_min", C.c_int64), ("wave_max", C.c_int64), ("wg_cost", C.c_int64),
                ("extent_mean_max", C.c_int64), ("small_piece_min", C.c_int64), ("cus", C.c_int32),
                ("wave_kib", C.c_int32), ("ragged_copy", C.c_int32), ("extent_copy", C.c_int32),
                ("small_pieces", C.c_int32), ("small_kib", C.c_int32), ("small_order", C.c_int32)]
    DEFAULTS = dict(chunk=32768, wave_min=1 << 20, wave_max=32 << 20, wg_cost=2048, extent_mean_max=1024,
                    small_piece_min=112 << 20, cus=256, wave_kib=0, ragged_copy=1, extent_copy=1, small_pieces=1,
                    small_kib=8, small_order=8)


class CopyChoice(C.Structure):
    """xg_copy_choice"""
    _fields_ = [("kind", C.c_int32), ("nt", C.c_int32), ("kib", C.c_int32), ("order", C.c_int32), ("piece", C.c_int64)]


COPY_PIECE, COPY_WAVE, COPY_SHIFT, COPY_EXTENT, COPY_SMALL, COPY_NKIND = range(6)   # xg_sched.h XG_COPY_*


class PlanKnobs(C.Structure):
    """xg_plan_knobs: every context setting the plan-table builder reads"""
    _fields_ = ([("rules", CopyRules)] +
                [(k, C.c_int64) for k in ("extent_tile", "engine_max_step", "solo_max", "launch_max", "split_min",
                                          "self_max")] +
                [(k, C.c_int32) for k in ("variant", "engine_wmax", "engine_drain", "solo", "solo_rails", "solo_waves",
                                          "wave_grid", "step_chain", "engine_arm", "fuse_stage", "split_after_pack",
                                          "rank", "nranks", "virt")])


class PlanTables:
    """The tables xg_plan_load builds from a device plan, built with no GPU (xg_plan_tables_build,
    csrc/host/plan_tables.cc).  dp: a DevPlan (or a pointer to one); base / nbytes: the regions'
    addresses and sizes (default: 2 MiB-aligned fake addresses, the plan's own region sizes);
    cus / engine_occ / wave_grid: the device facts xg_init queries (default: a whole MI355X; a
    context's own: Context.knobs()); env: the XG_* knobs a context would be opened under;
    knobs: xg_plan_knobs or xg_copy_rules fields by name, over both."""
    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:        # bound at first use: a libxghost without plan_tables.cc still serves the rest
            h = host()
            T, I = C.c_void_p, C.POINTER(C.c_int)
            h.xg_plan_knobs_default.restype = None
            h.xg_plan_knobs_default.argtypes = [C.POINTER(PlanKnobs), C.c_int, C.c_int, C.c_int]
            h.xg_plan_knobs_env.restype = None
            h.xg_plan_knobs_env.argtypes = [C.POINTER(PlanKnobs), C.POINTER(C.c_char_p)]
            h.xg_plan_knob_names.argtypes = [C.POINTER(C.c_char_p), C.c_int]
            h.xg_plan_tables_build.argtypes = [C.POINTER(DevPlan), C.POINTER(PlanKnobs), C.POINTER(C.c_uint64),
                                               C.POINTER(C.c_int64), C.POINTER(T)]
            h.xg_plan_tables_free.restype = None
            h.xg_plan_tables_free.argtypes = [T]
            for fn in ("nsteps", "launches", "shift_launches", "extent_launches", "engine", "engine_rails"):
                getattr(h, "xg_plan_tables_" + fn).argtypes = [T]
            h.xg_plan_tables_step_form.argtypes = [T, C.c_int]
            h.xg_plan_tables_kind_launches.argtypes = [T, C.c_int]
            h.xg_plan_tables_wave_launches.argtypes = [T, I, I]
            h.xg_plan_tables_small_launches.argtypes = [T, I]
            h.xg_plan_tables_engine_steps.argtypes = [T, I, I]
            h.xg_plan_tables_dump.restype = C.c_int64
            h.xg_plan_tables_dump.argtypes = [T, C.c_char_p, C.c_int64]
            cls._lib = h
        return cls._lib

    @classmethod
    def knob_names(cls):
        """the environment variables xg_plan_knobs_env reads"""
        out = (C.c_char_p * cls.lib().xg_plan_knob_names(None, 0))()
        cls.lib().xg_plan_knob_names(out, len(out))
        return [n.decode() for n in out]

    @classmethod
    def knobs(cls, cus=256, engine_occ=256, wave_grid=2048, env=None, **over):
        """the defaults, then env ({name: value}, parsed as xg_init parses the process environment, which
        is not touched; XG_GRAPH is no plan knob and passes, another unknown name raises), then over"""
        k = PlanKnobs()
        cls.lib().xg_plan_knobs_default(C.byref(k), cus, engine_occ, wave_grid)
        if env is not None:
            unknown = set(env) - set(cls.knob_names()) - {"XG_GRAPH"}
            if unknown:
                raise XGError("not a plan knob: %s" % ", ".join(sorted(unknown)))
            arr = [("%s=%s" % nv).encode() for nv in env.items()] + [None]
            cls.lib().xg_plan_knobs_env(C.byref(k), (C.c_char_p * len(arr))(*arr))
        rules = set(f[0] for f in CopyRules._fields_)
        for name, v in over.items():
            setattr(k.rules if name in rules else k, name, v)      # an unknown name raises (ctypes structures take no new fields)
            assert name in rules or name in set(f[0] for f in PlanKnobs._fields_), name
        return k

    def __init__(self, dp, base=None, nbytes=None, cus=256, engine_occ=256, wave_grid=2048, env=None, **knobs):
        h = self.lib()
        dpp = dp if isinstance(dp, C.POINTER(DevPlan)) else C.pointer(dp)
        self.base = list(base) if base is not None else [(b + 1) << 40 for b in range(NBUF)]
        self.nbytes = list(nbytes) if nbytes is not None else list(dpp.contents.region_bytes)
        self.h = C.c_void_p()
        k = self.knobs(cus, engine_occ, wave_grid, env, **knobs)
        rc = h.xg_plan_tables_build(dpp, C.byref(k), (C.c_uint64 * NBUF)(*self.base), (C.c_int64 * NBUF)(*self.nbytes),
                                    C.byref(self.h))
        if rc:
            raise XGError("xg_plan_tables_build: %d" % rc)

    def close(self):
        if self.h:
            self.lib().xg_plan_tables_free(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def nsteps(self):
        return self.lib().xg_plan_tables_nsteps(self.h)

    def launches(self):
        return self.lib().xg_plan_tables_launches(self.h)

    def step_form(self, s):
        return self.lib().xg_plan_tables_step_form(self.h, s)

    def kind_launches(self):
        return [self.lib().xg_plan_tables_kind_launches(self.h, k) for k in range(COPY_NKIND)]

    def engine_rails(self):
        return self.lib().xg_plan_tables_engine_rails(self.h)

    def engine(self):
        return self.lib().xg_plan_tables_engine(self.h)

    def engine_steps(self):
        """-> (steps inside segments, segments, hazard barriers)"""
        ns, nh = C.c_int(), C.c_int()
        n = self.lib().xg_plan_tables_engine_steps(self.h, C.byref(ns), C.byref(nh))
        return n, ns.value, nh.value

    def dump(self):
        return dump_tables(self.h)

    def records(self):
        return parse_tables(self.dump())


def dump_tables(handle):
    """xg_plan_tables_dump of a handle (a PlanTables', or xg_plan_tables_of a loaded plan)"""
    h = PlanTables.lib()
    n = h.xg_plan_tables_dump(handle, None, 0)
    buf = C.create_string_buffer(n + 1)
    h.xg_plan_tables_dump(handle, buf, n + 1)
    return buf.value.decode()


def parse_tables(text):
    """the dump by record tag: {"piece": [[fields...], ...], ...}.  A field that is a number is an
    int; a pointer "b+off" is the pair (b, off); a record's tag and index are dropped; of
    "name value" records (plan, step, launch, seg) the result is a dict."""
    def val(x):
        if "+" in x and x[0] != "?":
            b, o = x.split("+")
            return (int(b), int(o))
        try:
            return int(x, 0)
        except ValueError:
            return x
    out = {}
    for line in text.splitlines():
        f = line.split()
        tag = f[0]
        if tag in ("plan", "vec", "views"):
            out[tag] = dict((f[i], val(f[i + 1])) for i in range(1, len(f), 2))
        elif tag == "step":
            names = ("stage", "local", "pack", "post", "calls", "bytes", "l")
            d, i = {}, 2
            while i < len(f):
                width = 2 if f[i] in names[:5] else 4 if f[i] == "bytes" else 3 if f[i] == "l" else 1
                v = [val(x) for x in f[i + 1:i + 1 + width]]
                d[f[i]] = v[0] if width == 1 else v
                i += 1 + width
            out.setdefault("step", []).append(d)
        elif tag in ("launch", "seg", "call", "fix"):
            d, i = {}, 2
            while i < len(f):
                width = 5 if f[i] == "q" else 2 if f[i] == "steps" else 1
                v = [val(x) for x in f[i + 1:i + 1 + width]]
                d[f[i]] = v[0] if width == 1 else v
                i += 1 + width
            out.setdefault(tag, []).append(d)
        else:
            v = [val(x) for x in f[2:]]
            out.setdefault(tag, []).append(v[0] if len(v) == 1 else v)
    return out


class VecTables:
    """The tables xg_vecplace_load builds from a GPU's row list, built with no GPU
    (xg_vec_tables_build, csrc/host/vec_tables.cc).  rows: VRow records or (src_buf, dst_buf, src_off,
    dst_off, src_step, dst_step, len, count) tuples; nbytes: the regions' sizes (NBUF entries);
    base: their addresses (default: fake ones a TiB apart).  XGError when the builder refuses."""
    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            h = host()
            T, i64 = C.c_void_p, C.c_int64
            h.xg_vec_tables_build.argtypes = [C.POINTER(VRow), i64, C.POINTER(C.c_uint64), C.POINTER(i64), i64, C.c_int,
                                              i64, C.POINTER(T)]
            h.xg_vec_tables_free.restype = None
            h.xg_vec_tables_free.argtypes = [T]
            for fn in ("rows", "tiles", "bytes"):
                getattr(h, "xg_vec_tables_" + fn).restype = i64
                getattr(h, "xg_vec_tables_" + fn).argtypes = [T]
            h.xg_vec_tables_dispatches.argtypes = [T]
            for fn in ("cut", "dispatch_bytes"):
                getattr(h, "xg_vec_tables_" + fn).restype = i64
                getattr(h, "xg_vec_tables_" + fn).argtypes = [T, C.c_int]
            h.xg_vec_tables_dump.restype = i64
            h.xg_vec_tables_dump.argtypes = [T, C.c_char_p, i64]
            cls._lib = h
        return cls._lib

    def __init__(self, rows, nbytes, base=None, tile_bytes=32768, tile_pieces=256, launch_max=512 << 20):
        h = self.lib()
        arr, n = _vrow_array(rows)
        self.base = list(base) if base is not None else [(b + 1) << 40 for b in range(NBUF)]
        self.nbytes = list(nbytes) + [0] * (NBUF - len(nbytes))
        self.h = C.c_void_p()
        rc = h.xg_vec_tables_build(arr, n, (C.c_uint64 * NBUF)(*self.base), (C.c_int64 * NBUF)(*self.nbytes), tile_bytes,
                                   tile_pieces, launch_max, C.byref(self.h))
        if rc:
            raise XGError("xg_vec_tables_build: %d" % rc)

    def close(self):
        if self.h:
            self.lib().xg_vec_tables_free(self.h)
            self.h = C.c_void_p()

    __del__ = close

    @property
    def rows(self):
        return self.lib().xg_vec_tables_rows(self.h)

    @property
    def tiles(self):
        return self.lib().xg_vec_tables_tiles(self.h)

    @property
    def dispatches(self):
        return self.lib().xg_vec_tables_dispatches(self.h)

    @property
    def bytes(self):
        return self.lib().xg_vec_tables_bytes(self.h)

    def cuts(self):
        """the dispatches' tile boundaries: dispatches + 1 entries from 0 to tiles"""
        return [self.lib().xg_vec_tables_cut(self.h, k) for k in range(self.dispatches + 1)]

    def dispatch_bytes(self):
        return [self.lib().xg_vec_tables_dispatch_bytes(self.h, k) for k in range(self.dispatches)]

    def dump(self):
        h = self.lib()
        n = h.xg_vec_tables_dump(self.h, None, 0)
        buf = C.create_string_buffer(n + 1)
        h.xg_vec_tables_dump(self.h, buf, n + 1)
        return buf.value.decode()

    def records(self):
        """the dump by record tag, as parse_tables gives a plan's: "vec" a dict, "row" lists of
        [(buf, off) src, (buf, off) dst, src_step, dst_step, len, count], "tile0" / "cut" / "dbytes" ints"""
        return parse_tables(self.dump())


class ViewTables:
    """The tables xg_vecplace_load_views builds from a GPU's row list, built with no GPU
    (xg_view_tables_build, csrc/host/vec_tables.cc): the rows in view order, a record per view, tile0
    over the views, the dispatch cuts.  Arguments and XGError as VecTables."""
    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            h = host()
            T, i64 = C.c_void_p, C.c_int64
            h.xg_view_tables_build.argtypes = [C.POINTER(VRow), i64, C.POINTER(C.c_uint64), C.POINTER(i64), i64, C.c_int,
                                               i64, C.POINTER(T)]
            h.xg_view_tables_free.restype = None
            h.xg_view_tables_free.argtypes = [T]
            for fn in ("rows", "views", "multi", "tiles", "bytes"):
                getattr(h, "xg_view_tables_" + fn).restype = i64
                getattr(h, "xg_view_tables_" + fn).argtypes = [T]
            h.xg_view_tables_dispatches.argtypes = [T]
            for fn in ("cut", "dispatch_bytes"):
                getattr(h, "xg_view_tables_" + fn).restype = i64
                getattr(h, "xg_view_tables_" + fn).argtypes = [T, C.c_int]
            h.xg_view_tables_order.restype = i64
            h.xg_view_tables_order.argtypes = [T, i64]
            h.xg_view_tables_dump.restype = i64
            h.xg_view_tables_dump.argtypes = [T, C.c_char_p, i64]
            cls._lib = h
        return cls._lib

    def __init__(self, rows, nbytes, base=None, tile_bytes=32768, tile_pieces=256, launch_max=512 << 20):
        h = self.lib()
        arr, n = _vrow_array(rows)
        self.base = list(base) if base is not None else [(b + 1) << 40 for b in range(NBUF)]
        self.nbytes = list(nbytes) + [0] * (NBUF - len(nbytes))
        self.h = C.c_void_p()
        rc = h.xg_view_tables_build(arr, n, (C.c_uint64 * NBUF)(*self.base), (C.c_int64 * NBUF)(*self.nbytes), tile_bytes,
                                    tile_pieces, launch_max, C.byref(self.h))
        if rc:
            raise XGError("xg_view_tables_build: %d" % rc)

    def close(self):
        if self.h:
            self.lib().xg_view_tables_free(self.h)
            self.h = C.c_void_p()

    __del__ = close

    rows = property(lambda self: self.lib().xg_view_tables_rows(self.h))
    views = property(lambda self: self.lib().xg_view_tables_views(self.h), doc="all views")
    multi = property(lambda self: self.lib().xg_view_tables_multi(self.h), doc="the views of more than one row")
    tiles = property(lambda self: self.lib().xg_view_tables_tiles(self.h))
    dispatches = property(lambda self: self.lib().xg_view_tables_dispatches(self.h))
    bytes = property(lambda self: self.lib().xg_view_tables_bytes(self.h))

    def cuts(self):
        """the dispatches' tile boundaries: dispatches + 1 entries from 0 to tiles"""
        return [self.lib().xg_view_tables_cut(self.h, k) for k in range(self.dispatches + 1)]

    def dispatch_bytes(self):
        return [self.lib().xg_view_tables_dispatch_bytes(self.h, k) for k in range(self.dispatches)]

    def order(self):
        """the list index of every device row"""
        return [self.lib().xg_view_tables_order(self.h, i) for i in range(self.rows)]

    def dump(self):
        h = self.lib()
        n = h.xg_view_tables_dump(self.h, None, 0)
        buf = C.create_string_buffer(n + 1)
        h.xg_view_tables_dump(self.h, buf, n + 1)
        return buf.value.decode()

    def records(self):
        """the dump by record tag: "views" a dict, "row" as VecTables', "order" ints, "view" lists of
        [row0, k, jb, kind], "tile0" / "cut" / "dbytes" ints"""
        return parse_tables(self.dump())


class RunOpts(C.Structure):
    """xg_run_opts"""
    _fields_ = [("verify", C.c_int), ("fingerprint", C.c_int), ("eager_limit", C.c_int64),
                ("pack_max_seg", C.c_int64), ("proc_node", C.c_int), ("barrier_type", C.c_int),
                ("rep_timers", C.POINTER(Timer)), ("pack_min_bytes", C.c_int64), ("pack_form", C.c_int)]


A2M, M2A = 0, 1
BUF_SEND, BUF_RECV, BUF_STAGE_SEND, BUF_STAGE_RECV, BUF_SCRATCH = 0, 1, 2, 3, 4
PACK_TWO_SIDED, PACK_ONE_SIDED, RELAY, RELAY_COALESCED = 0, 1, 2, 3   # xg_devplan_build_form (xg_sched.h XG_RELAY, XG_RELAY_COALESCED)
CALL_SEND, CALL_RECV, CALL_BARRIER, CALL_FENCE = 1, 2, 3, 4   # xg_call kinds
MSG_COPY, MSG_COLL, MSG_CTRL = 1, 2, 4
DP_RAGGED = 1          # xg_devplan.flags bit 0 (XG_DP_RAGGED)
DP_EXTENTS = 2         # bit 1 (XG_DP_EXTENTS): a placement plan, short launches may run copy_kernel_x
EARG, ENOMEM = 3, 4    # XG_EARG, XG_ENOMEM
TAM_METHODS = (15, 16)
MPICH_EAGER_LIMIT = 65424


def _load(name):
    path = os.path.join(LIBDIR, name)
    if not os.path.exists(path):
        raise XGError("%s not built: run `make -C %s` (or __graft_entry__.build())" % (path, HERE))
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


_host = None
_dev = None


def host():
    global _host
    if _host is None:
        h = _load("libxghost.so")
        h.xg_aggregator_list.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        h.xg_method_label.restype = C.c_char_p
        h.xg_method_label.argtypes = [C.c_int]
        h.xg_method_direction.argtypes = [C.c_int]
        h.xg_sched_build.restype = C.c_void_p
        h.xg_sched_build.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int),
                                     C.c_int, C.c_int, C.c_int, C.c_int64, C.c_char_p, C.c_size_t]
        h.xg_sched_build_iter.restype = C.c_void_p
        h.xg_sched_build_iter.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int),
                                          C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_char_p, C.c_size_t]
        h.xg_sched_build_v.restype = C.c_void_p
        h.xg_sched_build_v.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int),
                                       C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_char_p, C.c_size_t]
        h.xg_sched_free.argtypes = [C.c_void_p]
        h.xg_sched_ragged.argtypes = [C.c_void_p]
        for fn in ("xg_seg_offset", "xg_slot_offset"):
            getattr(h, fn).restype = C.c_int64
            getattr(h, fn).argtypes = [C.c_void_p, C.c_int, C.c_int]
        h.xg_delivery_lens.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
        for fn in ("xg_sched_nmsg", "xg_sched_nsteps", "xg_sched_direction", "xg_sched_procs"):
            getattr(h, fn).argtypes = [C.c_void_p]
        h.xg_sched_msgs.restype = C.POINTER(Msg)
        h.xg_sched_msgs.argtypes = [C.c_void_p]
        h.xg_sched_trace.restype = C.c_size_t
        h.xg_sched_trace.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
        h.xg_sched_rank_timer.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double),
                                          C.POINTER(C.c_double), C.POINTER(Timer)]
        h.xg_sched_rank_rep_timers.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.POINTER(Timer)]
        h.xg_sched_ntimes.argtypes = [C.c_void_p]
        h.xg_sched_timed_steps.argtypes = [C.c_void_p, C.POINTER(C.c_uint8)]
        h.xg_sched_barrier_epochs.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        h.xg_save_all_timing.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(Timer), C.c_char_p]
        h.xg_block_range.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        h.xg_gpu_of.argtypes = [C.c_int, C.c_int, C.c_int]
        for fn in ("xg_send_offset", "xg_recv_offset", "xg_scratch_offset"):
            getattr(h, fn).restype = C.c_int64
            getattr(h, fn).argtypes = [C.c_void_p, C.c_int, C.c_int]
        h.xg_region_bytes.restype = C.c_int64
        h.xg_region_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        h.xg_devplan_build.restype = C.POINTER(DevPlan)
        h.xg_devplan_build.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64]
        h.xg_devplan_build_ex.restype = C.POINTER(DevPlan)
        h.xg_devplan_build_ex.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64]
        h.xg_devplan_build_form.restype = C.POINTER(DevPlan)
        h.xg_devplan_build_form.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int]
        h.xg_devplan_free.argtypes = [C.POINTER(DevPlan)]
        h.xg_devplan_step_calls.argtypes = [C.POINTER(DevPlan), C.c_int, C.c_int64, C.POINTER(Call)]
        h.xg_devplan_step_self_calls.argtypes = [C.POINTER(DevPlan), C.c_int, C.c_int64]
        h.xg_calls_match.restype = C.c_int64
        h.xg_calls_match.argtypes = [C.c_int, C.c_int, C.POINTER(C.POINTER(Call)), C.POINTER(C.POINTER(C.c_int32)),
                                     C.POINTER(CallPair), C.c_int64, C.c_char_p, C.c_size_t]
        h.xg_devplans_match.restype = C.c_int64
        h.xg_devplans_match.argtypes = [C.POINTER(C.POINTER(DevPlan)), C.c_int, C.c_int64, C.POINTER(CallPair),
                                        C.c_int64, C.c_char_p, C.c_size_t]
        h.xg_step_local_meets_unpacks.argtypes = [C.POINTER(DevPlan), C.c_int]
        h.xg_step_packs_meet_unpacks.argtypes = [C.POINTER(DevPlan), C.c_int]
        h.xg_step_stage_meets_rest.argtypes = [C.POINTER(DevPlan), C.c_int]
        h.xg_piece_size.restype = C.c_int64
        h.xg_piece_size.argtypes = [C.POINTER(C.c_int64), C.c_int, C.c_int64, C.c_int, C.c_int64]
        h.xg_extent_tiles.argtypes = [C.POINTER(C.c_int64), C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int32)]
        h.xg_small_piece_at.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int] + [C.POINTER(C.c_int64)] * 3
        # the step engines' counter arithmetic (xg_sched.h xg_eng_*): uint32 in, uint32 or a truth value out
        u32 = C.c_uint32
        for fn, nargs, res in (("xg_eng_grid_pre_target", 2, u32), ("xg_eng_grid_target", 3, u32),
                               ("xg_eng_waiting", 2, C.c_int), ("xg_eng_last", 2, C.c_int),
                               ("xg_eng_solo_lines", 1, u32), ("xg_eng_solo_per_line", 2, u32),
                               ("xg_eng_solo_arrive_target", 2, u32), ("xg_eng_solo_line_last", 4, C.c_int),
                               ("xg_eng_solo_rails_last", 3, C.c_int)):
            getattr(h, fn).argtypes = [u32] * nargs
            getattr(h, fn).restype = res
        h.xg_eng_grid_tickets.argtypes = [u32, u32, C.c_int]
        h.xg_eng_grid_tickets.restype = u32
        h.xg_eng_solo_state_after.argtypes = [u32, u32, C.POINTER(EngSoloState)]
        h.xg_eng_solo_state_after.restype = None
        h.xg_launch_facts_add.restype = None
        h.xg_launch_facts_add.argtypes = [C.POINTER(LaunchFacts), C.POINTER(Copy)]
        h.xg_copy_launch_choose.argtypes = [C.POINTER(LaunchFacts), C.POINTER(CopyRules), C.POINTER(CopyChoice)]
        h.xg_exts_lens.argtypes = [C.POINTER(Ext), C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        h.xg_exts_check.argtypes = [C.POINTER(Ext), C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int,
                                    C.c_char_p, C.c_size_t]
        h.xg_domain_offset.restype = C.c_int64
        h.xg_domain_offset.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        h.xg_domain_bytes.restype = C.c_int64
        h.xg_domain_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        h.xg_place_plan_build.restype = C.POINTER(DevPlan)
        h.xg_place_plan_build.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Ext), C.c_int64, C.POINTER(C.c_int64)]
        h.xg_vecs_expand.argtypes = [C.POINTER(Vec), C.c_int64, C.POINTER(Ext), C.c_int64]
        h.xg_vecs_expand.restype = C.c_int64
        h.xg_vecs_lens.argtypes = [C.POINTER(Vec), C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        h.xg_vecs_check.argtypes = [C.POINTER(Vec), C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int,
                                    C.c_char_p, C.c_size_t]
        h.xg_vec_rows_build.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Vec), C.c_int64, C.POINTER(C.c_int64),
                                        C.POINTER(VRow), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        h.xg_vec_rows_build.restype = C.c_int64
        h.xg_vec_row_tiles.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int]
        h.xg_vec_row_tiles.restype = C.c_int64
        h.xg_vec_piece.argtypes = [C.POINTER(VRow), C.c_int64, C.c_int, C.c_int64, C.c_int] + [C.POINTER(C.c_int64)] * 3
        h.xg_vec_rows_tiles.argtypes = [C.POINTER(VRow), C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_int32)]
        h.xg_vec_rows_tiles.restype = C.c_int64
        h.xg_vrow_views.argtypes = [C.POINTER(VRow), C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        h.xg_vrow_views.restype = C.c_int64
        h.xg_view_tiles.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int]
        h.xg_view_tiles.restype = C.c_int64
        h.xg_view_piece.argtypes = [C.POINTER(VRow), C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int)] + \
            [C.POINTER(C.c_int64)] * 3
        h.xg_fill_runs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(SegRun)]
        h.xg_verify_slots.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Slot)]
        h.xg_deliveries.argtypes = [C.c_void_p, C.c_int, C.POINTER(Delivery)]
        h.xg_engine_hazards.argtypes = [C.POINTER(Span), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]
        h.xg_engine_rail_safe.argtypes = [C.POINTER(Span), C.POINTER(C.c_int), C.c_int]
        h.xg_solo_reduce_stamps.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int64, C.c_int, C.c_int,
                                            C.POINTER(C.c_uint64)]
        h.xg_solo_reduce_stamps.restype = None
        h.xg_solo_tables.argtypes = [C.POINTER(Span), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_uint64,
                                     C.c_uint64, C.POINTER(SoloShape), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        h.xg_solo_tables_g.argtypes = [C.POINTER(Span), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_uint64, C.c_uint64, C.POINTER(SoloShape), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_int)]
        h.xg_summarize_results.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_char_p, Timer, Timer]
        _host = h
    return _host


def aggregator_list(procs, cb_nodes, proc_node=1, agg_type=1):
    rl = (C.c_int * cb_nodes)()
    if host().xg_aggregator_list(procs, cb_nodes, proc_node, agg_type, rl) != 0:
        raise XGError("aggregator type %d is not defined by the reference" % agg_type)
    return list(rl)


def engine_hazards(steps, force=False):
    """xg_engine_hazards over steps = [[(src, dst, len), ...], ...] (byte addresses):
    returns (flags per step, number of hazard points)."""
    spans = [x for st in steps for x in st]
    arr = (Span * max(1, len(spans)))(*[Span(*x) for x in spans])
    beg = [0]
    for st in steps:
        beg.append(beg[-1] + len(st))
    sb = (C.c_int * len(beg))(*beg)
    fl = (C.c_int * max(1, len(steps)))()
    n = host().xg_engine_hazards(arr, sb, len(steps), 1 if force else 0, fl)
    return list(fl)[:len(steps)], n


def rail_safe(steps):
    """xg_engine_rail_safe over steps = [[(src, dst, len), ...], ...]: may they run on the solo
    engine's unsynchronised rails (no source range meets another step's destination range)?"""
    spans = [x for st in steps for x in st]
    arr = (Span * max(1, len(spans)))(*[Span(*x) for x in spans])
    beg = [0]
    for st in steps:
        beg.append(beg[-1] + len(st))
    sb = (C.c_int * len(beg))(*beg)
    return bool(host().xg_engine_rail_safe(arr, sb, len(steps)))


def solo_tables(steps, rails_max, src_base, dst_base, waves=16, granule=16):
    """xg_solo_tables_g over steps = [[(src, dst, len), ...], ...]: returns (rc, shape dict,
    per-rail descriptor lists, per-rail row barrier counts, per-rail closed-step lists,
    per-rail rows holding real pieces)."""
    spans = [x for st in steps for x in st]
    arr = (Span * max(1, len(spans)))(*[Span(*x) for x in spans])
    beg = [0]
    for st in steps:
        beg.append(beg[-1] + len(st))
    sb = (C.c_int * len(beg))(*beg)
    sh = SoloShape()
    rc = host().xg_solo_tables_g(arr, sb, len(steps), rails_max, waves, granule, src_base, dst_base, C.byref(sh),
                                 None, None)
    shape = {"rails": sh.rails, "npieces": sh.npieces, "nrows": sh.nrows, "nmeta": sh.nmeta}
    if rc:
        return rc, shape, None, None, None, None
    R, npc, nr, n = sh.rails, sh.npieces, sh.nrows, len(steps)
    d = (C.c_uint64 * (R * npc))()
    m = (C.c_int * sh.nmeta)()
    rc = host().xg_solo_tables_g(arr, sb, n, rails_max, waves, granule, src_base, dst_base, C.byref(sh), d, m)
    descs = [list(d[r * npc:(r + 1) * npc]) for r in range(R)]
    close = [list(m[r * (nr + 1):(r + 1) * (nr + 1)]) for r in range(R)]
    off = R * (nr + 1)
    csteps = [list(m[off + r * n: off + (r + 1) * n]) for r in range(R)]
    rows = list(m[off + R * n: off + R * n + R])
    return rc, shape, descs, close, csteps, rows


def solo_reduce_stamps(stamps, s0, s1):
    """xg_solo_reduce_stamps over stamps = [rail][step] (ints, 0 = nothing closed)"""
    R, n = len(stamps), len(stamps[0])
    arr = (C.c_uint64 * (R * n))(*[x for row in stamps for x in row])
    out = (C.c_uint64 * n)()
    host().xg_solo_reduce_stamps(arr, R, n, s0, s1, out)
    return list(out)


def solo_rail_last(steps, rails):
    """xg_solo_rail_last over steps = [[(src, dst, len), ...], ...] -> each rail's last step with pieces"""
    spans = [x for st in steps for x in st]
    arr = (Span * max(1, len(spans)))(*[Span(*x) for x in spans])
    beg = [0]
    for st in steps:
        beg.append(beg[-1] + len(st))
    fn = host().xg_solo_rail_last
    fn.argtypes = [C.POINTER(Span), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int32)]
    out = (C.c_int32 * rails)()
    rc = fn(arr, (C.c_int * len(beg))(*beg), len(steps), rails, out)
    if rc:
        raise XGError("xg_solo_rail_last: %d" % rc)
    return list(out)


def solo_carry_tail(stamps, csteps, last):
    """xg_solo_carry_tail over stamps = [rail][step] of one segment, csteps = the tables' per-rail
    closed-step lists, last = xg_solo_rail_last -> the stamps with the sat-out tail steps zeroed"""
    R, n = len(stamps), len(stamps[0])
    arr = (C.c_uint64 * (R * n))(*[x for row in stamps for x in row])
    fn = host().xg_solo_carry_tail
    fn.restype = None
    fn.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int32)]
    fn(arr, R, n, 0, n, (C.c_int * (R * n))(*[x for row in csteps for x in row]), (C.c_int32 * R)(*last))
    return [list(arr[r * n:(r + 1) * n]) for r in range(R)]


def step_times(marks, seg_of, seg_end, wall_hz, chain_stamps=None, engine_stamps=None, chain_end=None,
               need_mark=None, host_total=-1.0):
    """xg_step_times: step_done[] (seconds) from a run's stamps (64-bit ints); marks = [start,
    boundary 0, ...] (None for an armed run, host_total >= 0), the other lists one entry per step
    or None -> (rc, step_done)"""
    n = len(seg_of)

    def arr(t, v):
        return (t * max(1, len(v)))(*v) if v is not None else None
    u64, i32 = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    fn = host().xg_step_times
    fn.argtypes = [C.c_int, u64, u64, u64, i32, i32, i32, C.POINTER(C.c_uint8), C.c_double, C.c_double,
                   C.POINTER(C.c_double)]
    out = (C.c_double * max(1, n))()
    rc = fn(n, arr(C.c_uint64, marks), arr(C.c_uint64, chain_stamps), arr(C.c_uint64, engine_stamps),
            arr(C.c_int32, seg_of), arr(C.c_int32, seg_end), arr(C.c_int32, chain_end), arr(C.c_uint8, need_mark),
            wall_hz, host_total, out)
    return rc, list(out)[:n]


def _pairs(n, arr, groups=False):
    if groups:
        return [(q.step, q.group, q.src, q.dst, q.send_call, q.recv_call, q.len) for q in arr[:n]]
    return [(q.step, q.src, q.dst, q.send_call, q.recv_call, q.len) for q in arr[:n]]


def calls_match(calls, nsteps):
    """xg_calls_match over calls[g] = [[(kind, peer, buf, off, len), ...] per step]: RCCL's
    pairing of a G-GPU job's calls; returns [(step, src, dst, send_call, recv_call, len)]
    (step-major) or raises XGError with the reason."""
    G = len(calls)
    arrs, begs = [], []
    for g in range(G):
        flat = [c for st in calls[g] for c in st]
        a = (Call * max(1, len(flat)))(*[Call(k, p, b, 0, o, n) for k, p, b, o, n in flat])
        beg = [0]
        for st in calls[g]:
            beg.append(beg[-1] + len(st))
        arrs.append(a)
        begs.append((C.c_int32 * len(beg))(*beg))
    ca = (C.POINTER(Call) * G)(*[C.cast(a, C.POINTER(Call)) for a in arrs])
    cb = (C.POINTER(C.c_int32) * G)(*[C.cast(b, C.POINTER(C.c_int32)) for b in begs])
    err = C.create_string_buffer(512)
    n = host().xg_calls_match(G, nsteps, ca, cb, None, 0, err, 512)
    if n < 0:
        raise XGError(err.value.decode())
    out = (CallPair * max(1, n))()
    host().xg_calls_match(G, nsteps, ca, cb, out, n, err, 512)
    return _pairs(n, out)


def devplans_match(plans, self_max=0, groups=False):
    """xg_devplans_match over the G device plans (DevicePlanView or raw POINTER(DevPlan)) of one
    job (calls listed with self_max): the pairs (groups: (step, group, src, dst, send_call,
    recv_call, len)), or XGError naming the first call that RCCL would pair differently."""
    ptrs = [p.ptr if isinstance(p, DevicePlanView) else p for p in plans]
    G = len(ptrs)
    arr = (C.POINTER(DevPlan) * G)(*ptrs)
    err = C.create_string_buffer(512)
    n = host().xg_devplans_match(arr, G, self_max, None, 0, err, 512)
    if n < 0:
        raise XGError(err.value.decode())
    out = (CallPair * max(1, n))()
    host().xg_devplans_match(arr, G, self_max, out, n, err, 512)
    return _pairs(n, out, groups)


def piece_size(lens, chunk=32768, cus=256, wg_cost=2048):
    """xg_piece_size: the workgroup piece size of one copy launch over copies of these lengths"""
    arr = (C.c_int64 * max(1, len(lens)))(*lens)
    return host().xg_piece_size(arr, len(lens), chunk, cus, wg_cost)


def extent_tiles(lens, tile_bytes=32768, tile_pieces=256):
    """xg_extent_tiles: the tiles of one copy_kernel_x dispatch over pieces of these lengths, as the
    list of tile boundaries (count + 1 entries); None for a cap < 1"""
    n = len(lens)
    arr = (C.c_int64 * max(1, n))(*lens)
    nt = host().xg_extent_tiles(arr, n, tile_bytes, tile_pieces, None)
    if nt < 0:
        return None
    begin = (C.c_int32 * (nt + 1))()
    assert host().xg_extent_tiles(arr, n, tile_bytes, tile_pieces, begin) == nt
    return list(begin)


def launch_facts(copies, dp_flags=0, cross=False, may_small=False, nt_cut=False, nt_run=False):
    """xg_launch_facts of one copy launch over copies = [(src_buf, src_off, dst_buf, dst_off, len)],
    gathered as plan load gathers them (xg_launch_facts_add per copy)"""
    f = LaunchFacts()
    f._lens = (C.c_int64 * max(1, len(copies)))(*[c[4] for c in copies])
    for sb, so, db, do, n in copies:
        host().xg_launch_facts_add(C.byref(f), C.byref(Copy(so, do, n, sb, db)))
    f.lens, f.nlens = C.cast(f._lens, C.POINTER(C.c_int64)), len(copies)
    f.dp_flags, f.cross, f.may_small, f.nt_cut, f.nt_run = dp_flags, cross, may_small, nt_cut, nt_run
    return f


def copy_launch_choose(facts, **rules):
    """xg_copy_launch_choose: the kernel kind of one copy launch -> (kind, nt, kib, order, piece
    bytes), or None when it refuses (a launch without bytes); rules: fields of CopyRules over
    its DEFAULTS"""
    r, ch = CopyRules(**dict(CopyRules.DEFAULTS, **rules)), CopyChoice()
    if host().xg_copy_launch_choose(C.byref(facts), C.byref(r), C.byref(ch)) != 0:
        return None
    return ch.kind, ch.nt, ch.kib, ch.order, ch.piece


def small_piece_at(b, copies, length, piece, k=1):
    """xg_small_piece_at: (copy, offset, bytes) of workgroup b of a small-piece launch (copy_kernel_q) over
    `copies` copies of `length` bytes in pieces of `piece` bytes, k copies to a group; None when b is
    no workgroup of it"""
    out = [C.c_int64() for _ in range(3)]
    if host().xg_small_piece_at(b, copies, length, piece, k, *[C.byref(x) for x in out]) != 0:
        return None
    return tuple(x.value for x in out)


def _ext_array(exts):
    """exts: Ext records or (rank, agg, off, len) tuples -> (C array, n)"""
    v = [e if isinstance(e, Ext) else Ext(*[int(x) for x in e]) for e in exts]
    return (Ext * max(1, len(v)))(*v), len(v)


def exts_lens(exts, procs, cb_nodes):
    """xg_exts_lens: the P x A length matrix (row-major) of an extent list; XGError when refused"""
    arr, n = _ext_array(exts)
    out = (C.c_int64 * (procs * cb_nodes))()
    if host().xg_exts_lens(arr, n, procs, cb_nodes, out) != 0:
        raise XGError("xg_exts_lens: rank or aggregator out of range, negative length or overflow")
    return list(out)


def exts_check(exts, procs, cb_nodes, dom_bytes, scatter=True):
    """xg_exts_check -> (code, reason): (0, "") for a list that may be placed (scatter: as a
    collective write, where extents of one aggregator may not overlap)"""
    arr, n = _ext_array(exts)
    dom = (C.c_int64 * max(1, cb_nodes))(*[int(x) for x in dom_bytes])
    err = C.create_string_buffer(512)
    rc = host().xg_exts_check(arr, n, procs, cb_nodes, dom, 1 if scatter else 0, err, 512)
    return rc, err.value.decode()


def _vec_array(vecs):
    """vecs: Vec records or (rank, agg, off, len, stride, count) tuples -> (C array, n)"""
    v = [e if isinstance(e, Vec) else Vec(*[int(x) for x in e]) for e in vecs]
    return (Vec * max(1, len(v)))(*v), len(v)


def _vrow_array(rows):
    """rows: VRow records or (src_buf, dst_buf, src_off, dst_off, src_step, dst_step, len, count) tuples"""
    v = [r if isinstance(r, VRow) else VRow(*[int(x) for x in r]) for r in rows]
    return (VRow * max(1, len(v)))(*v), len(v)


def vecs_expand(vecs):
    """xg_vecs_expand: the extent list a vec list means, as (rank, agg, off, len) tuples -- one per
    block of every positive vec, in order (O(blocks): the definition, not a fast path); None when
    it refuses (a negative len, count or stride, or an offset or count past int64)"""
    arr, n = _vec_array(vecs)
    m = host().xg_vecs_expand(arr, n, None, 0)
    if m < 0:
        return None
    out = (Ext * max(1, m))()
    assert host().xg_vecs_expand(arr, n, out, m) == m
    return [(e.rank, e.agg, e.off, e.len) for e in out[:m]]


def vecs_lens(vecs, procs, cb_nodes):
    """xg_vecs_lens: the P x A length matrix (row-major) of a vec list; XGError when refused"""
    arr, n = _vec_array(vecs)
    out = (C.c_int64 * (procs * cb_nodes))()
    if host().xg_vecs_lens(arr, n, procs, cb_nodes, out) != 0:
        raise XGError("xg_vecs_lens: rank or aggregator out of range, negative length or count, or overflow")
    return list(out)


def vecs_check(vecs, procs, cb_nodes, dom_bytes, scatter=True):
    """xg_vecs_check -> (code, reason): what exts_check says of the expansion, without building it"""
    arr, n = _vec_array(vecs)
    dom = (C.c_int64 * max(1, cb_nodes))(*[int(x) for x in dom_bytes])
    err = C.create_string_buffer(512)
    rc = host().xg_vecs_check(arr, n, procs, cb_nodes, dom, 1 if scatter else 0, err, 512)
    return rc, err.value.decode()


def vec_row_tiles(length, count, tile_bytes=32768, tile_pieces=256):
    """xg_vec_row_tiles: the tiles (one workgroup each) of one row of a strided placement"""
    return host().xg_vec_row_tiles(length, count, tile_bytes, tile_pieces)


def vec_piece_at(row, t, i, tile_bytes=32768, tile_pieces=256):
    """xg_vec_piece: (src_off, dst_off, n) of lane i of tile t of a row (n = 0 past the tile's last
    piece); None when t is no tile of the row or i no lane"""
    arr, _n = _vrow_array([row])
    out = [C.c_int64() for _ in range(3)]
    if host().xg_vec_piece(arr, tile_bytes, tile_pieces, t, i, *[C.byref(x) for x in out]) != 0:
        return None
    return tuple(x.value for x in out)


def vec_rows_tiles(rows, tile_bytes=32768, tile_pieces=256):
    """xg_vec_rows_tiles: the prefix sums of the rows' tile counts (len(rows) + 1 entries); None
    when the total passes 2^31 - 1"""
    arr, n = _vrow_array(rows)
    t0 = (C.c_int32 * (n + 1))()
    if host().xg_vec_rows_tiles(arr, n, tile_bytes, tile_pieces, t0) < 0:
        return None
    return list(t0)


VIEW_SINGLE, VIEW_DST_STRIPED, VIEW_SRC_STRIPED = 0, 1, 2      # XG_VIEW_*


def vrow_views(rows, tile_bytes=32768, tile_pieces=256):
    """xg_vrow_views: the rows of a list grouped into views -> [(kind, [list indices of the view's
    rows, ascending on the striped side])], in view order"""
    arr, n = _vrow_array(rows)
    order, k, kind = (C.c_int64 * max(1, n))(), (C.c_int32 * max(1, n))(), (C.c_int32 * max(1, n))()
    nv = host().xg_vrow_views(arr, n, tile_bytes, tile_pieces, order, k, kind)
    if nv < 0:
        raise XGError("xg_vrow_views: bad arguments or out of host memory")
    out, at = [], 0
    for v in range(nv):
        out.append((kind[v], list(order[at:at + k[v]])))
        at += k[v]
    assert at == n
    return out


def view_tiles(length, count, k, tile_bytes=32768, tile_pieces=256):
    """xg_view_tiles: the tiles (one workgroup each) of a view of k rows"""
    return host().xg_view_tiles(length, count, k, tile_bytes, tile_pieces)


def view_piece(rows, t, q, tile_bytes=32768, tile_pieces=256):
    """xg_view_piece: (row, src_off, dst_off, n) of lane q of tile t of the view made of `rows` (in
    view order, or a VRow array made once for many calls; n = 0: the lane is idle); None when the rows
    are no view, t is no tile of it or q no lane"""
    arr, k = (rows, len(rows)) if isinstance(rows, C.Array) else _vrow_array(rows)
    row, out = C.c_int(), [C.c_int64() for _ in range(3)]
    if host().xg_view_piece(arr, k, tile_bytes, tile_pieces, t, q, C.byref(row), *[C.byref(x) for x in out]) != 0:
        return None
    return (row.value,) + tuple(x.value for x in out)


def method_label(method):
    lab = host().xg_method_label(method)
    return lab.decode() if lab else None


class Schedule:
    """One method run (all -k repetitions), compiled to device-wide steps."""

    def __init__(self, method, procs, cb_nodes, data_size, comm_size, rank_list, ntimes=1,
                 eager_limit=MPICH_EAGER_LIMIT, proc_node=1, barrier_type=0, iteration=0, lens=None):
        """lens: a length per (rank, aggregator index) pair, row-major P x A (xg_sched_build_v;
        data_size is then unused and self.d is the longest segment, or the common one)."""
        h = host()
        self.method, self.P, self.A, self.d, self.c = method, procs, cb_nodes, data_size, comm_size
        self.rank_list = list(rank_list)
        self.ntimes = ntimes
        err = C.create_string_buffer(512)
        rl = (C.c_int * cb_nodes)(*rank_list)
        if lens is not None:
            flat = [int(x) for x in lens]
            if len(flat) != procs * cb_nodes:
                raise XGError("lens must have procs * cb_nodes = %d entries, not %d" % (procs * cb_nodes, len(flat)))
            self.lens = flat
            self.d = max(flat) if flat else 0
            self._h = h.xg_sched_build_v(method, procs, cb_nodes, (C.c_int64 * max(1, len(flat)))(*flat), comm_size,
                                         rl, ntimes, proc_node, barrier_type, eager_limit, iteration, err, 512)
        else:
            self.lens = None
            self._h = h.xg_sched_build_iter(method, procs, cb_nodes, data_size, comm_size, rl, ntimes,
                                            proc_node, barrier_type, eager_limit, iteration, err, 512)
        if not self._h:
            raise XGError(err.value.decode())
        self.nsteps = h.xg_sched_nsteps(self._h)
        self.direction = h.xg_sched_direction(self._h)
        self.ragged = bool(h.xg_sched_ragged(self._h))

    def __del__(self):
        if getattr(self, "_h", None) and _host is not None:
            _host.xg_sched_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def messages(self):
        n = host().xg_sched_nmsg(self._h)
        ptr = host().xg_sched_msgs(self._h)
        return [(m.src, m.sseg, m.dst, m.dslot, m.len, m.step, m.flags) for m in ptr[:n]]

    def locations(self):
        """Per message: (sbuf, soff, dbuf, doff) -- region and offset inside the rank's part."""
        n = host().xg_sched_nmsg(self._h)
        ptr = host().xg_sched_msgs(self._h)
        return [(m.sbuf, m.soff, m.dbuf, m.doff) for m in ptr[:n]]

    def trace(self, rank):
        n = host().xg_sched_trace(self._h, rank, None, 0)
        buf = C.create_string_buffer(n + 1)
        host().xg_sched_trace(self._h, rank, buf, n + 1)
        return buf.value.decode()

    def timed_steps(self):
        """per step 1 if some rank's Timer reads its completion time (the last step always),
        else 0 -- the steps a timed run must mark (xg_sched_timed_steps)"""
        need = (C.c_uint8 * max(1, self.nsteps))()
        if host().xg_sched_timed_steps(self._h, need) < 0:
            raise XGError("xg_sched_timed_steps failed")
        return list(need)[:self.nsteps]

    def rank_timer(self, rank, step_done, step_post=None, ngpus=1):
        nd = (C.c_double * max(1, len(step_done)))(*step_done)
        npost = (C.c_double * max(1, len(step_post)))(*step_post) if step_post is not None else None
        t = Timer()
        if host().xg_sched_rank_timer(self._h, ngpus, rank, nd, npost, C.byref(t)) != 0:
            raise XGError("xg_sched_rank_timer: bad rank/ngpus")
        return t

    def rank_rep_timers(self, rank, step_done, step_post=None, ngpus=1):
        """timers[m] of every repetition (m13)."""
        nd = (C.c_double * max(1, len(step_done)))(*step_done)
        npost = (C.c_double * max(1, len(step_post)))(*step_post) if step_post is not None else None
        reps = (Timer * max(1, self.ntimes))()
        if host().xg_sched_rank_rep_timers(self._h, ngpus, rank, nd, npost, reps) != 0:
            raise XGError("xg_sched_rank_rep_timers: bad rank/ngpus")
        return list(reps)[:self.ntimes]

    def barrier_epochs(self):
        n = host().xg_sched_barrier_epochs(self._h, None)
        out = (C.c_int32 * max(1, n))()
        host().xg_sched_barrier_epochs(self._h, out)
        return list(out)[:n]

    def gpu_of(self, ngpus, rank):
        return host().xg_gpu_of(self.P, ngpus, rank)

    def block_range(self, ngpus, g):
        lo, hi = C.c_int(), C.c_int()
        host().xg_block_range(self.P, ngpus, g, C.byref(lo), C.byref(hi))
        return lo.value, hi.value

    def send_offset(self, ngpus, rank):
        return host().xg_send_offset(self._h, ngpus, rank)

    def recv_offset(self, ngpus, rank):
        return host().xg_recv_offset(self._h, ngpus, rank)

    def seg_offset(self, rank, seg):
        """byte offset of segment seg inside the rank's SEND part (xg_seg_offset)"""
        return host().xg_seg_offset(self._h, rank, seg)

    def slot_offset(self, rank, slot):
        """byte offset of slot `slot` inside the rank's RECV part (xg_slot_offset)"""
        return host().xg_slot_offset(self._h, rank, slot)

    def delivery_lens(self, ngpus):
        """xg_delivery_lens: the length of every delivery, in deliveries() order"""
        n = host().xg_delivery_lens(self._h, ngpus, None)
        out = (C.c_int64 * max(1, n))()
        host().xg_delivery_lens(self._h, ngpus, out)
        return list(out[:n])

    def scratch_offset(self, ngpus, rank):
        return host().xg_scratch_offset(self._h, ngpus, rank)

    def region_bytes(self, ngpus, g, buf):
        return host().xg_region_bytes(self._h, ngpus, g, buf)

    def devplan(self, ngpus, g, pack_max_seg=4 << 20, pack_min=0, pack_form=-1):
        return DevicePlanView(self, ngpus, g, pack_max_seg, pack_min, pack_form)

    def place_plan(self, ngpus, g, exts, dom_bytes):
        """xg_place_plan_build: GPU g's placement plan of this (exchange) schedule for an extent
        list, as a DevicePlanView (one step, one copy per hosted positive extent, in list order)"""
        arr, n = _ext_array(exts)
        dom = (C.c_int64 * max(1, self.A))(*[int(x) for x in dom_bytes])
        p = host().xg_place_plan_build(self._h, ngpus, g, arr, n, dom)
        if not p:
            raise XGError("xg_place_plan_build: out of host memory, or a rank / aggregator out of range")
        return DevicePlanView(self, ngpus, g, 0, plan=p)

    def vec_rows(self, ngpus, g, vecs, dom_bytes):
        """xg_vec_rows_build: GPU g's rows of this (exchange) schedule for a vec list -> (rows as
        (src_buf, dst_buf, src_off, dst_off, src_step, dst_step, len, count) tuples, the list index of
        every row, region_bytes)"""
        arr, n = _vec_array(vecs)
        dom = (C.c_int64 * max(1, self.A))(*[int(x) for x in dom_bytes])
        rb = (C.c_int64 * NBUF)()
        m = host().xg_vec_rows_build(self._h, ngpus, g, arr, n, dom, None, None, rb)
        if m < 0:
            raise XGError("xg_vec_rows_build: out of host memory, or a rank / aggregator out of range")
        rows, idx = (VRow * max(1, m))(), (C.c_int64 * max(1, m))()
        assert host().xg_vec_rows_build(self._h, ngpus, g, arr, n, dom, rows, idx, None) == m
        return ([tuple(getattr(r, f) for f, _t in VRow._fields_) for r in rows[:m]], list(idx)[:m], list(rb))

    def domain_offset(self, ngpus, a, dom_bytes):
        """xg_domain_offset: where aggregator index a's domain starts in its GPU's domain buffer"""
        dom = (C.c_int64 * max(1, self.A))(*[int(x) for x in dom_bytes])
        return host().xg_domain_offset(self._h, ngpus, a, dom)

    def domain_bytes(self, ngpus, g, dom_bytes):
        """xg_domain_bytes: the size of GPU g's domain buffer"""
        dom = (C.c_int64 * max(1, self.A))(*[int(x) for x in dom_bytes])
        return host().xg_domain_bytes(self._h, ngpus, g, dom)

    def check_pairing(self, ngpus, pack_max_seg=4 << 20, pack_min=0, pack_form=-1, self_max=0):
        """Refuse (XGError) a job whose GPUs' RCCL calls RCCL would not pair step by step
        (xg_devplans_match over every GPU's plan, built in C, the calls listed with the
        self_max the runtime posts with); returns the number of pairs."""
        h = host()
        plans = [h.xg_devplan_build_form(self._h, ngpus, g, pack_max_seg, pack_min, pack_form)
                 for g in range(ngpus)]
        try:
            if not all(plans):
                raise XGError("method %d on %d GPUs: out of host memory building the device plans"
                              % (self.method, ngpus))
            arr = (C.POINTER(DevPlan) * ngpus)(*plans)
            err = C.create_string_buffer(512)
            n = h.xg_devplans_match(arr, ngpus, self_max, None, 0, err, 512)
            if n < 0:
                raise XGError("method %d on %d GPUs: RCCL calls do not pair: %s"
                              % (self.method, ngpus, err.value.decode()))
            return n
        finally:
            for q in plans:
                if q:
                    h.xg_devplan_free(q)

    def fill_runs(self, ngpus, g):
        n = host().xg_fill_runs(self._h, ngpus, g, None)
        runs = (SegRun * max(1, n))()
        host().xg_fill_runs(self._h, ngpus, g, runs)
        return [(r.rank, r.seed0, r.off, r.nsegs) for r in runs[:n]]

    def verify_slots(self, ngpus, g):
        n = host().xg_verify_slots(self._h, ngpus, g, None)
        sl = (Slot * max(1, n))()
        host().xg_verify_slots(self._h, ngpus, g, sl)
        return [(x.src, x.seed, x.dst, x.off) for x in sl[:n]]

    def deliveries(self, ngpus):
        """xg_deliveries: every receive slot of the job with the send segment it must equal, as
        Delivery records (src, seed, dst, slot, src_gpu, dst_gpu, send_off, recv_off)"""
        n = host().xg_deliveries(self._h, ngpus, None)
        out = (Delivery * max(1, n))()
        host().xg_deliveries(self._h, ngpus, out)
        return list(out[:n])


class DevicePlanView:
    """Python view of xg_devplan (host memory), used by the CPU plan tests."""

    def __init__(self, sched, ngpus, g, pack_max_seg, pack_min=0, pack_form=-1, plan=None):
        self.sched = sched
        # pack_form: PACK_TWO_SIDED, PACK_ONE_SIDED, RELAY, RELAY_COALESCED, or -1 = the library's
        # default (xg_sched.h); plan: a built xg_devplan to view and own (Schedule.place_plan)
        self._p = plan or host().xg_devplan_build_form(sched.handle, ngpus, g, pack_max_seg, pack_min, pack_form)
        if not self._p:
            self._p = None
            raise XGError("xg_devplan_build_form: out of host memory")
        p = self._p.contents
        self.gpu, self.ngpus, self.nsteps = p.gpu, p.ngpus, p.nsteps
        self.flags = p.flags
        self.region_bytes = list(p.region_bytes)
        self.copies = [(c.src_buf, c.src_off, c.dst_buf, c.dst_off, c.len) for c in p.copies[:p.ncopy]]
        # (peer, is_send, region, offset, length, group): group 1 = a relay step's second RCCL group
        self.p2p = [(o.peer, o.is_send, o.buf, o.off, o.len, o.group) for o in p.p2p[:p.np2p]]
        self.steps = [(s.pre_begin, s.pre_count, s.p2p_begin, s.p2p_count, s.post_begin, s.post_count)
                      for s in p.steps[:p.nsteps]]
        self.sync_after = [s.sync_after for s in p.steps[:p.nsteps]]
        self.stage_count = [s.stage_count for s in p.steps[:p.nsteps]]
        self.posts = [s.posts for s in p.steps[:p.nsteps]]         # request posts of this GPU's ranks
        self.local_bytes = p.local_bytes
        self.remote_send_bytes = p.remote_send_bytes
        self.remote_recv_bytes = p.remote_recv_bytes

    @property
    def ptr(self):
        return self._p

    def local_meets_unpacks(self, step):
        """xg_step_local_meets_unpacks: may step's local copies share a launch with step-1's unpacks?"""
        return host().xg_step_local_meets_unpacks(self._p, step)

    def packs_meet_unpacks(self, step):
        """xg_step_packs_meet_unpacks: does a pack of step forward bytes step-1's unpacks write?"""
        return host().xg_step_packs_meet_unpacks(self._p, step)

    def stage_meets_rest(self, step):
        """xg_step_stage_meets_rest: must step's stage copies keep a launch of their own?"""
        return host().xg_step_stage_meets_rest(self._p, step)

    def calls(self, step, self_max=0):
        """xg_devplan_step_calls: [(kind, peer, buf, off, len)] this GPU posts in `step`"""
        n = host().xg_devplan_step_calls(self._p, step, self_max, None)
        arr = (Call * max(1, n))()
        host().xg_devplan_step_calls(self._p, step, self_max, arr)
        return [(c.kind, c.peer, c.buf, c.off, c.len) for c in arr[:n]]

    def __del__(self):
        if getattr(self, "_p", None) and _host is not None:
            _host.xg_devplan_free(self._p)
            self._p = None


# --------------------------------------------------------------------------- device (libxg.so)
ROCM_RUNTIME_LIBS = ("libamdhip64.so", "librccl.so", "libhsa-runtime64.so")


def foreign_rocm_runtime():
    """ROCm runtime libraries mapped into this process from outside the ROCm install libxg.so is
    built against (lib/rocm_libdir, /opt/rocm*, or $ROCM_PATH).  torch's wheel bundles its own libamdhip64.so.7,
    librccl.so.1 and libhsa-runtime64.so.1 under the same sonames: once `import torch` has
    loaded them, libxg.so binds to those instead -- another runtime and RCCL than it was built
    and tested with (the full GPU suite hung in RCCL that way, profiles/r04/torch_runtime/)."""
    roots = {os.path.realpath(r) for r in ("/opt/rocm", os.environ.get("ROCM_PATH") or "/opt/rocm")}
    try:        # the library directory of the ROCm libxg.so was linked against (written by the Makefile)
        roots.add(os.path.realpath(open(os.path.join(HERE, "lib", "rocm_libdir")).read().strip()))
    except OSError:
        pass
    try:
        roots |= {os.path.realpath(os.path.join("/opt", n)) for n in os.listdir("/opt") if n.startswith("rocm")}
        maps = open("/proc/self/maps").read().splitlines()
    except OSError:
        return []
    bad = set()
    for line in maps:
        path = line.split(None, 5)[5].strip() if len(line.split(None, 5)) == 6 else ""
        if os.path.basename(path).startswith(ROCM_RUNTIME_LIBS):
            rp = os.path.realpath(path)
            if not any(rp.startswith(r + os.sep) for r in roots):
                bad.add(rp)
    return sorted(bad)


def device():
    """libxg.so -- the HIP/RCCL half.  Loading it does not touch the GPU.  Refused (XGError) in a
    process that already holds another ROCm runtime (foreign_rocm_runtime: e.g. torch's)."""
    global _dev
    if _dev is None:
        host()
        bad = foreign_rocm_runtime()
        if bad:
            raise XGError("libxg.so would bind to the ROCm runtime already loaded in this process from %s "
                          "(e.g. by `import torch`), not the one it is built against: load the framework "
                          "before torch, or in a process without it" % ", ".join(bad))
        d = _load("libxg.so")
        # ... and after loading it: a foreign runtime found first on the library search path
        # (LD_LIBRARY_PATH) binds libxg.so's own dependencies to it
        d.xg_foreign_runtime.argtypes = [C.c_char_p, C.c_size_t]
        buf = C.create_string_buffer(1024)
        if d.xg_foreign_runtime(buf, 1024) > 0:
            raise XGError("libxg.so is bound to a ROCm runtime from outside /opt/rocm (%s): refused"
                          % buf.value.decode())
        vp, ip, i64 = C.c_void_p, C.c_int, C.c_int64
        d.xg_get_unique_id.argtypes = [vp]
        d.xg_init.argtypes = [C.POINTER(vp), ip, ip, ip, vp]
        d.xg_finalize.argtypes = [vp]
        d.xg_init_virtual.argtypes = [C.POINTER(vp), ip, ip, ip]
        d.xg_vplans_run.argtypes = [C.POINTER(vp), ip, C.POINTER(C.c_double)]
        d.xg_vplans_run_rccl.argtypes = [C.POINTER(vp), ip, C.POINTER(C.c_double)]
        d.xg_plan_set_local_only.argtypes = [vp, ip]
        d.xg_plan_engine_preset.argtypes = [vp, C.c_uint, C.c_uint]
        d.xg_plan_set_step_marks.argtypes = [vp, C.POINTER(C.c_uint8)]
        d.xg_self_max.restype = i64
        d.xg_self_max.argtypes = [vp]
        d.xg_ctx_knobs.argtypes = [vp, C.POINTER(PlanKnobs)]
        d.xg_barrier.argtypes = [vp]
        d.xg_sync.argtypes = [vp]
        d.xg_device_sync.argtypes = [vp]
        d.xg_allreduce_max.argtypes = [vp, C.POINTER(C.c_double), ip]
        d.xg_device_info.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(ip), C.POINTER(C.c_size_t)]
        d.xg_now.restype = C.c_double
        d.xg_regions_alloc.argtypes = [vp, C.POINTER(i64), C.POINTER(vp)]
        d.xg_regions_adopt.argtypes = [vp, C.POINTER(i64), vp, vp, C.POINTER(vp)]
        d.xg_chk_spans.argtypes = [vp, C.POINTER(BufSpan), ip, C.POINTER(C.c_uint64)]
        d.xg_is_virtual.argtypes = [vp]
        d.xg_run_opts_default.argtypes = [C.POINTER(RunOpts)]
        d.xg_run_opts_default.restype = None
        d.xg_exchange.argtypes = [vp, ip, ip, ip, ip, C.POINTER(ip), ip, vp, vp, C.POINTER(Timer), ip, ip,
                                  C.POINTER(RunOpts), C.POINTER(i64), C.c_char_p, C.c_size_t]
        d.xg_exchange_v.argtypes = [vp, ip, ip, ip, C.POINTER(i64), C.POINTER(ip), ip, vp, vp, C.POINTER(Timer), ip,
                                    ip, C.POINTER(RunOpts), C.POINTER(i64), C.c_char_p, C.c_size_t]
        d.xg_regions_free.argtypes = [vp]
        d.xg_regions_poison.argtypes = [vp]
        d.xg_regions_ptr.restype = vp
        d.xg_regions_ptr.argtypes = [vp, ip]
        d.xg_regions_read.argtypes = [vp, ip, i64, vp, i64]
        d.xg_regions_write.argtypes = [vp, ip, i64, vp, i64]
        d.xg_fill.argtypes = [vp, C.POINTER(SegRun), ip, i64, ip, ip]
        d.xg_verify.argtypes = [vp, C.POINTER(Slot), ip, i64, ip, ip, C.POINTER(C.c_uint64),
                                C.POINTER(i64), C.POINTER(i64)]
        d.xg_plan_load.argtypes = [vp, vp, C.POINTER(DevPlan), C.POINTER(vp)]
        d.xg_plan_free.argtypes = [vp]
        d.xg_plan_nsteps.argtypes = [vp]
        d.xg_plan_run.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        d.xg_plan_enqueue.argtypes = [vp]
        d.xg_plan_engine.argtypes = [vp]
        d.xg_plan_engine_rails.argtypes = [vp]
        d.xg_plan_check.argtypes = [vp]
        d.xg_plan_launches.argtypes = [vp]
        d.xg_plan_step_form.argtypes = [vp, ip]
        d.xg_plan_engine_steps.argtypes = [vp, C.POINTER(ip), C.POINTER(ip)]
        d.xg_plan_kind_launches.argtypes = [vp, ip]
        d.xg_plan_wave_launches.argtypes = [vp, C.POINTER(ip), C.POINTER(ip)]
        d.xg_plan_shift_launches.argtypes = [vp]
        d.xg_plan_extent_launches.argtypes = [vp]
        d.xg_plan_small_launches.argtypes = [vp, C.POINTER(ip)]
        d.xg_exchange_w.argtypes = [vp, ip, ip, ip, C.POINTER(Ext), i64, C.POINTER(i64), C.POINTER(ip), ip, vp, vp,
                                    C.POINTER(Timer), ip, ip, C.POINTER(RunOpts), C.POINTER(i64), C.POINTER(i64),
                                    C.POINTER(C.c_double), C.c_char_p, C.c_size_t]
        d.xg_exchange_wv.argtypes = [vp, ip, ip, ip, C.POINTER(Vec), i64, C.POINTER(i64), C.POINTER(ip), ip, vp, vp,
                                     C.POINTER(Timer), ip, ip, C.POINTER(RunOpts), C.POINTER(i64), C.POINTER(i64),
                                     C.POINTER(C.c_double), C.c_char_p, C.c_size_t]
        d.xg_exchange_wv_tiles.restype = i64
        d.xg_exchange_wv_tiles.argtypes = []
        d.xg_vecplace_load.argtypes = [vp, vp, C.POINTER(VRow), i64, C.POINTER(vp)]
        d.xg_vecplace_run.argtypes = [vp, C.POINTER(C.c_double)]
        d.xg_vecplace_free.argtypes = [vp]
        d.xg_vecplace_tiles.restype = i64
        d.xg_vecplace_tiles.argtypes = [vp]
        d.xg_vecplace_dispatches.argtypes = [vp]
        d.xg_vecplace_load_views.argtypes = [vp, vp, C.POINTER(VRow), i64, C.POINTER(vp)]
        d.xg_vecplace_views.restype = i64
        d.xg_vecplace_views.argtypes = [vp]
        d.xg_exchange_wv_views.restype = i64
        d.xg_exchange_wv_views.argtypes = []
        d.xg_plan_displs.argtypes = [vp, C.POINTER(i64), ip]
        d.xg_ktime_begin.argtypes = [vp, ip, ip]
        d.xg_ktime_end.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(ip), C.POINTER(i64)]
        d.xg_ktime_launch.argtypes = [vp, ip, C.POINTER(C.c_double), C.POINTER(i64)]
        d.xg_set_copy_params.argtypes = [vp, i64, ip]
        d.xg_p2p_bench.argtypes = [vp, i64, ip, ip, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        d.xg_p2p_pair_bench.argtypes = [vp, i64, ip, ip, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        d.xg_p2p_split_bench.argtypes = [vp, i64, ip, ip, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        d.xg_rccl_version.argtypes = [C.POINTER(C.c_int)]
        _dev = d
    return _dev


def _check(rc, what):
    if rc != 0:
        raise XGError("%s failed with code %d (see stderr)" % (what, rc))


def rccl_version():
    """ncclGetVersion of the RCCL libxg.so runs on, e.g. 22703 (no GPU call)"""
    v = C.c_int()
    _check(device().xg_rccl_version(C.byref(v)), "xg_rccl_version")
    return v.value


def unique_id():
    buf = C.create_string_buffer(128)
    _check(device().xg_get_unique_id(buf), "xg_get_unique_id")
    return buf.raw


class Context:
    """One process = one GPU (xg_init).  nranks > 1 needs rank 0's unique_id()."""

    def __init__(self, rank=0, nranks=1, device_index=None, uid=None, device=None):
        d = globals()["device"]()
        dev = device if device is not None else (device_index if device_index is not None else rank)
        self._c = C.c_void_p()
        ub = C.create_string_buffer(uid, 128) if uid else None
        _check(d.xg_init(C.byref(self._c), rank, nranks, dev, ub), "xg_init")
        self.rank, self.nranks = rank, nranks
        self.is_virtual = False

    @classmethod
    def virtual(cls, rank, nranks, device=0):
        """GPU `rank` of an `nranks`-GPU job emulated on one physical device (test hook,
        xg_init_virtual); run the job's plans together with run_virtual()."""
        self = cls.__new__(cls)
        self._c = C.c_void_p()
        _check(globals()["device"]().xg_init_virtual(C.byref(self._c), rank, nranks, device), "xg_init_virtual")
        self.rank, self.nranks = rank, nranks
        self.is_virtual = True
        return self

    @property
    def handle(self):
        return self._c

    def knobs(self):
        """the PlanKnobs this context loads plans with (xg_ctx_knobs)"""
        k = PlanKnobs()
        _check(_dev.xg_ctx_knobs(self._c, C.byref(k)), "xg_ctx_knobs")
        return k

    def barrier(self):
        _check(_dev.xg_barrier(self._c), "xg_barrier")

    def sync(self):
        _check(_dev.xg_sync(self._c), "xg_sync")

    def device_sync(self):
        _check(_dev.xg_device_sync(self._c), "xg_device_sync")

    def allreduce_max(self, vals):
        arr = (C.c_double * len(vals))(*vals)
        _check(_dev.xg_allreduce_max(self._c, arr, len(vals)), "xg_allreduce_max")
        return list(arr)

    def info(self):
        name = C.create_string_buffer(64)
        cus, hbm = C.c_int(), C.c_size_t()
        _check(_dev.xg_device_info(self._c, name, 64, C.byref(cus), C.byref(hbm)), "xg_device_info")
        return name.value.decode(), cus.value, hbm.value

    def set_copy_params(self, chunk=0, variant=0):
        _check(_dev.xg_set_copy_params(self._c, chunk, variant), "xg_set_copy_params")

    def p2p_bench(self, nbytes, mode=0, reps=20):
        g, sec = C.c_double(), C.c_double()
        _check(_dev.xg_p2p_bench(self._c, nbytes, mode, reps, C.byref(g), C.byref(sec)), "xg_p2p_bench")
        return g.value, sec.value

    def p2p_split_bench(self, nbytes, calls, reps=20):
        """all pairs, every transfer of `nbytes` posted as `calls` calls -> (GB/s sent, s per rep)"""
        g, sec = C.c_double(), C.c_double()
        _check(_dev.xg_p2p_split_bench(self._c, nbytes, calls, reps, C.byref(g), C.byref(sec)),
               "xg_p2p_split_bench")
        return g.value, sec.value

    def p2p_pair_bench(self, nbytes, peer, reps=10):
        """one link, both directions at once, with `peer` (< 0: idle this round) -> (GB/s sent, s per rep)"""
        g, sec = C.c_double(), C.c_double()
        _check(_dev.xg_p2p_pair_bench(self._c, nbytes, peer, reps, C.byref(g), C.byref(sec)), "xg_p2p_pair_bench")
        return g.value, sec.value

    def ktime_begin(self, max_launches=4096, per_launch=True):
        """per_launch: an event pair around every copy / engine launch; else one pair
        around the whole session on the main stream (launches and bytes counted)."""
        _check(_dev.xg_ktime_begin(self._c, max_launches, 1 if per_launch else 2), "xg_ktime_begin")

    def ktime_end(self):
        ms, n, b = C.c_double(), C.c_int(), C.c_int64()
        _check(_dev.xg_ktime_end(self._c, C.byref(ms), C.byref(n), C.byref(b)), "xg_ktime_end")
        return ms.value, n.value, b.value

    def ktime_launches(self, n):
        """per-launch (ms, algorithmic bytes) of the last kernel-timing session"""
        out = []
        for k in range(n):
            ms, b = C.c_double(), C.c_int64()
            _check(_dev.xg_ktime_launch(self._c, k, C.byref(ms), C.byref(b)), "xg_ktime_launch")
            out.append((ms.value, b.value))
        return out

    def close(self):
        if self._c:
            _check(_dev.xg_finalize(self._c), "xg_finalize")
            self._c = None


def now():
    return device().xg_now()


def plan_wave_launches(plan):
    """xg_plan_wave_launches of a loaded plan handle -> (launches, grid, max pieces per wave)"""
    g, m = C.c_int(), C.c_int()
    n = device().xg_plan_wave_launches(plan, C.byref(g), C.byref(m))
    return n, g.value, m.value


def plan_kind_launches(plan):
    """xg_plan_kind_launches of a loaded plan handle for every kind -> [PIECE, WAVE, SHIFT, EXTENT, SMALL]"""
    return [device().xg_plan_kind_launches(plan, k) for k in range(COPY_NKIND)]


FORM_SPLIT, FORM_FUSED, FORM_FUSED_LOCAL, FORM_STAGE_FUSED, FORM_DEFERRED, FORM_SELF_LOCAL, FORM_ENGINE = (
    1, 2, 4, 8, 16, 32, 64)            # xg.h XG_FORM_*


def plan_step_form(plan, step):
    """xg_plan_step_form of a loaded plan handle: the XG_FORM_* bits of step `step`"""
    return device().xg_plan_step_form(plan, step)


def plan_engine_segments(plan):
    """the engine segments of a loaded plan handle (xg_plan_engine_steps' *nseg), each one launch"""
    nseg = C.c_int()
    device().xg_plan_engine_steps(plan, C.byref(nseg), None)
    return nseg.value


def run_virtual(runs, rccl=False):
    """Execute the MethodRuns of every GPU of one virtual job (runs[g] on Context.virtual(g, n))
    step by step on one device; returns step_done[] (device seconds).  rccl: move the
    cross-GPU pairs through RCCL (1-rank communicator, self send/recv) instead of copies."""
    n = len(runs)
    arr = (C.c_void_p * n)(*[r._p for r in runs])
    nst = max(1, runs[0].nsteps)
    done = (C.c_double * nst)()
    fn = "xg_vplans_run_rccl" if rccl else "xg_vplans_run"
    _check(getattr(device(), fn)(arr, n, done), fn)
    return list(done)[:runs[0].nsteps]


class Regions:
    """HBM regions (xg_regions_alloc) that several MethodRuns may reuse in turn: at
    hundreds of GiB, allocating and freeing per method costs seconds (the driver
    clears fresh pages), refilling and re-poisoning costs milliseconds."""

    def __init__(self, ctx, region_bytes):
        self.bytes = list(region_bytes)
        rb = (C.c_int64 * NBUF)(*self.bytes)
        self._r = C.c_void_p()
        _check(device().xg_regions_alloc(ctx.handle, rb, C.byref(self._r)), "xg_regions_alloc")

    @classmethod
    def adopt(cls, ctx, region_bytes, send=None, recv=None):
        """Regions whose SEND / RECV are the caller's device memory (addresses as int; None:
        allocated here): xg_regions_adopt.  Nothing is written to adopted memory, close() frees
        only what the library allocated."""
        self = cls.__new__(cls)
        self.bytes = list(region_bytes)
        rb = (C.c_int64 * NBUF)(*self.bytes)
        self._r = C.c_void_p()
        _check(device().xg_regions_adopt(ctx.handle, rb, C.c_void_p(send), C.c_void_p(recv), C.byref(self._r)),
               "xg_regions_adopt")
        return self

    def fits(self, region_bytes):
        return all(a <= b for a, b in zip(region_bytes, self.bytes))

    def ptr(self, buf):
        """device address of a region (int; 0 for an empty one)"""
        return _dev.xg_regions_ptr(self._r, buf) or 0

    def read(self, buf, off, length):
        out = C.create_string_buffer(max(1, length))
        _check(_dev.xg_regions_read(self._r, buf, off, out, length), "xg_regions_read")
        return out.raw[:length]

    def write(self, buf, off, data):
        b = C.create_string_buffer(bytes(data), len(data))
        _check(_dev.xg_regions_write(self._r, buf, off, b, len(data)), "xg_regions_write")

    def close(self):
        if getattr(self, "_r", None):
            _check(_dev.xg_regions_free(self._r), "xg_regions_free")
            self._r = None


def chk_spans(regions_or_run, spans):
    """xg_chk_spans: xg_chk64 of every (buf, off, len) span of a Regions' or MethodRun's regions,
    in one kernel launch"""
    n = len(spans)
    arr = (BufSpan * max(1, n))(*[BufSpan(b, 0, o, ln) for b, o, ln in spans])
    out = (C.c_uint64 * max(1, n))()
    _check(device().xg_chk_spans(regions_or_run._r, arr, n, out), "xg_chk_spans")
    return list(out)[:n]


def payload_check(runs):
    """The runs of one job (a MethodRun, or the G runs of a virtual job, in GPU order) after its
    exchange: every receive slot's checksum against its source segment's in the owning run's
    SEND (Schedule.deliveries) -- bytes the library need not know.  Returns the bad (dst, slot)."""
    runs = [runs] if isinstance(runs, MethodRun) else list(runs)
    G = len(runs)
    dl = runs[0].sched.deliveries(G)
    ln = runs[0].sched.delivery_lens(G)
    src, dst = [None] * len(dl), [None] * len(dl)
    for g, run in enumerate(runs):
        ks = [k for k, q in enumerate(dl) if q.src_gpu == g]
        for k, c in zip(ks, chk_spans(run, [(BUF_SEND, dl[k].send_off, ln[k]) for k in ks])):
            src[k] = c
        kr = [k for k, q in enumerate(dl) if q.dst_gpu == g]
        for k, c in zip(kr, chk_spans(run, [(BUF_RECV, dl[k].recv_off, ln[k]) for k in kr])):
            dst[k] = c
    return [(q.dst, q.slot) for k, q in enumerate(dl) if src[k] != dst[k]]


def exchange(ctx, method, procs, cb_nodes, data_size, rank_list, comm_size, send, recv, it=0, ntimes=1,
             verify=True, proc_node=1, pack_form=-1):
    """xg_exchange: the method's exchange over the caller's device buffers (addresses as int, laid
    out as Schedule.send_offset / recv_offset / region_bytes say).  Returns (rc, bad_slots,
    [Timer of every hosted rank], error text); raises nothing, so that every rank of a job sees
    the code."""
    d = device()
    o = RunOpts()
    d.xg_run_opts_default(C.byref(o))
    o.verify, o.proc_node = 1 if verify else 0, proc_node
    if pack_form >= 0:
        o.pack_form = pack_form
    lo, hi = C.c_int(), C.c_int()
    host().xg_block_range(procs, ctx.nranks, ctx.rank, C.byref(lo), C.byref(hi))
    timers = (Timer * max(1, hi.value - lo.value))()
    rl = (C.c_int * cb_nodes)(*rank_list)
    bad = C.c_int64()
    err = C.create_string_buffer(512)
    rc = d.xg_exchange(ctx.handle, method, procs, cb_nodes, data_size, rl, comm_size, C.c_void_p(send),
                       C.c_void_p(recv), timers, it, ntimes, C.byref(o), C.byref(bad), err, 512)
    return rc, bad.value, list(timers)[:hi.value - lo.value], err.value.decode()


def exchange_v(ctx, method, procs, cb_nodes, lens, rank_list, comm_size, send, recv, it=0, ntimes=1,
               verify=True, proc_node=1, pack_form=-1):
    """xg_exchange_v: xg_exchange with a length per (rank, aggregator index) pair (lens: row-major
    P x A) in place of data_size; buffers laid out as a Schedule(..., lens=) says.  Returns what
    exchange() returns."""
    d = device()
    o = RunOpts()
    d.xg_run_opts_default(C.byref(o))
    o.verify, o.proc_node = 1 if verify else 0, proc_node
    if pack_form >= 0:
        o.pack_form = pack_form
    lo, hi = C.c_int(), C.c_int()
    host().xg_block_range(procs, ctx.nranks, ctx.rank, C.byref(lo), C.byref(hi))
    timers = (Timer * max(1, hi.value - lo.value))()
    rl = (C.c_int * cb_nodes)(*rank_list)
    flat = [int(x) for x in lens]
    if len(flat) != procs * cb_nodes:
        raise XGError("lens must have procs * cb_nodes = %d entries, not %d" % (procs * cb_nodes, len(flat)))
    la = (C.c_int64 * max(1, len(flat)))(*flat)
    bad = C.c_int64()
    err = C.create_string_buffer(512)
    rc = d.xg_exchange_v(ctx.handle, method, procs, cb_nodes, la, rl, comm_size, C.c_void_p(send),
                         C.c_void_p(recv), timers, it, ntimes, C.byref(o), C.byref(bad), err, 512)
    return rc, bad.value, list(timers)[:hi.value - lo.value], err.value.decode()


def exchange_w(ctx, method, procs, cb_nodes, exts, dom_bytes, rank_list, comm_size, send, recv, it=0, ntimes=1,
               verify=True, proc_node=1, pack_form=-1):
    """xg_exchange_w: xg_exchange_v with the aggregator side placed by the extent list (a2m: send =
    dense ragged SEND, recv = this GPU's domain buffer; m2a: send = the domain buffer, recv = dense
    ragged RECV; addresses as int).  Returns (rc, bad_slots, bad_exts, place_s, [Timer of every
    hosted rank], error text); raises nothing, so that every rank of a job sees the code."""
    d = device()
    o = RunOpts()
    d.xg_run_opts_default(C.byref(o))
    o.verify, o.proc_node = 1 if verify else 0, proc_node
    if pack_form >= 0:
        o.pack_form = pack_form
    lo, hi = C.c_int(), C.c_int()
    host().xg_block_range(procs, ctx.nranks, ctx.rank, C.byref(lo), C.byref(hi))
    timers = (Timer * max(1, hi.value - lo.value))()
    rl = (C.c_int * cb_nodes)(*rank_list)
    arr, n = _ext_array(exts)
    dom = (C.c_int64 * max(1, cb_nodes))(*[int(x) for x in dom_bytes])
    bad, bad_e, place_s = C.c_int64(), C.c_int64(), C.c_double()
    err = C.create_string_buffer(512)
    rc = d.xg_exchange_w(ctx.handle, method, procs, cb_nodes, arr, n, dom, rl, comm_size, C.c_void_p(send),
                         C.c_void_p(recv), timers, it, ntimes, C.byref(o), C.byref(bad), C.byref(bad_e),
                         C.byref(place_s), err, 512)
    return rc, bad.value, bad_e.value, place_s.value, list(timers)[:hi.value - lo.value], err.value.decode()


class PlaceRun:
    """One GPU's placement step on its own: the placement plan of a schedule and an extent list
    (Schedule.place_plan) loaded over regions whose SEND / RECV are the caller's (addresses as int)
    or allocated here.  a2m: SEND = the dense RECV layout of the exchange, RECV = the domain
    buffer; m2a: SEND = the domain buffer, RECV = the dense SEND layout."""

    def __init__(self, ctx, sched, exts, dom_bytes, send=None, recv=None):
        d = device()
        self.ctx, self.sched = ctx, sched
        self.view = sched.place_plan(ctx.nranks, ctx.rank, exts, dom_bytes)
        # the list index of every hosted positive extent, in the plan's copy order
        self.ext_index = [i for i, e in enumerate(_ext_array(exts)[0][:len(exts)])
                          if e.len > 0 and sched.gpu_of(ctx.nranks, sched.rank_list[e.agg]) == ctx.rank]
        self.regions = Regions.adopt(ctx, self.view.region_bytes, send=send, recv=recv)
        self._r = self.regions._r
        self._p = C.c_void_p()
        _check(d.xg_plan_load(ctx.handle, self._r, self.view.ptr, C.byref(self._p)), "xg_plan_load")

    def run(self):
        """one timed run -> the placement step's device seconds"""
        done, post, wall = (C.c_double * 1)(), (C.c_double * 1)(), C.c_double()
        _check(_dev.xg_plan_run(self._p, done, post, C.byref(wall)), "xg_plan_run")
        return done[0]

    def extent_launches(self):
        """copy launches that run copy_kernel_x (xg_plan_extent_launches)"""
        return _dev.xg_plan_extent_launches(self._p)

    def shift_launches(self):
        return _dev.xg_plan_shift_launches(self._p)

    @property
    def launches(self):
        return _dev.xg_plan_launches(self._p)

    def close(self):
        if getattr(self, "_p", None):
            _check(_dev.xg_plan_free(self._p), "xg_plan_free")
            self._p = None
        if getattr(self, "regions", None):
            self.regions.close()
            self.regions = None


def place_check(run):
    """A PlaceRun after its run: xg_chk_spans of every hosted extent on both sides of the placement
    (one launch per side).  Returns the list indices of the extents whose sides differ."""
    cp = run.view.copies
    src = chk_spans(run, [(sb, so, n) for (sb, so, _db, _do, n) in cp])
    dst = chk_spans(run, [(db, do, n) for (_sb, _so, db, do, n) in cp])
    return [run.ext_index[k] for k in range(len(cp)) if src[k] != dst[k]]


def exchange_wv(ctx, method, procs, cb_nodes, vecs, dom_bytes, rank_list, comm_size, send, recv, it=0, ntimes=1,
                verify=True, proc_node=1, pack_form=-1):
    """xg_exchange_wv: exchange_w with the placement described by strided runs (Vec records or (rank,
    agg, off, len, stride, count) tuples), placed by one copy_kernel_v launch.  Returns (rc, bad_slots,
    bad_vecs, place_s, [Timer of every hosted rank], error text), as exchange_w does; vec_tiles() then
    tells how many copy_kernel_v workgroups the placement ran (0: it went by the expansion)."""
    d = device()
    o = RunOpts()
    d.xg_run_opts_default(C.byref(o))
    o.verify, o.proc_node = 1 if verify else 0, proc_node
    if pack_form >= 0:
        o.pack_form = pack_form
    lo, hi = C.c_int(), C.c_int()
    host().xg_block_range(procs, ctx.nranks, ctx.rank, C.byref(lo), C.byref(hi))
    timers = (Timer * max(1, hi.value - lo.value))()
    rl = (C.c_int * cb_nodes)(*rank_list)
    arr, n = _vec_array(vecs)
    dom = (C.c_int64 * max(1, cb_nodes))(*[int(x) for x in dom_bytes])
    bad, bad_v, place_s = C.c_int64(), C.c_int64(), C.c_double()
    err = C.create_string_buffer(512)
    rc = d.xg_exchange_wv(ctx.handle, method, procs, cb_nodes, arr, n, dom, rl, comm_size, C.c_void_p(send),
                          C.c_void_p(recv), timers, it, ntimes, C.byref(o), C.byref(bad), C.byref(bad_v),
                          C.byref(place_s), err, 512)
    return rc, bad.value, bad_v.value, place_s.value, list(timers)[:hi.value - lo.value], err.value.decode()


def vec_tiles():
    """xg_exchange_wv_tiles: the copy_kernel_v workgroups of this process's last exchange_wv placement"""
    return device().xg_exchange_wv_tiles()


def exchange_wv_views():
    """xg_exchange_wv_views: the views of more than one row of this process's last exchange_wv
    placement (0 unless XG_VEC_VIEWS=1 loaded it by views)"""
    return device().xg_exchange_wv_views()


class VecPlace:
    """One GPU's strided placement on its own: rows (VRow records or tuples; Schedule.vec_rows gives
    a vec list's) loaded as one copy_kernel_v launch (xg_vecplace_load) or, with views=True, as one
    copy_kernel_vv launch over the list's views (xg_vecplace_load_views), over regions of region_bytes
    whose SEND / RECV are the caller's (addresses as int) or allocated here.  XGError for rows the
    host builder refuses: nothing has run then."""

    def __init__(self, ctx, rows, region_bytes, send=None, recv=None, vec_index=None, views=False):
        d = device()
        self.ctx = ctx
        self.rows = [r if isinstance(r, VRow) else VRow(*[int(x) for x in r]) for r in rows]
        self.vec_index = list(vec_index) if vec_index is not None else list(range(len(self.rows)))
        rb = list(region_bytes) + [0] * (NBUF - len(region_bytes))
        self.regions = Regions.adopt(ctx, rb, send=send, recv=recv)
        self._r = self.regions._r
        self._v = C.c_void_p()
        arr, n = _vrow_array(self.rows)
        load = d.xg_vecplace_load_views if views else d.xg_vecplace_load
        rc = load(ctx.handle, self._r, arr, n, C.byref(self._v))
        if rc:
            self.regions.close()
            self.regions = None
            raise XGError("xg_vecplace_load%s failed with code %d (see stderr)" % ("_views" if views else "", rc))

    def run(self):
        """one timed run -> the launch's device seconds"""
        t = C.c_double()
        _check(_dev.xg_vecplace_run(self._v, C.byref(t)), "xg_vecplace_run")
        return t.value

    @property
    def tiles(self):
        return _dev.xg_vecplace_tiles(self._v)

    @property
    def dispatches(self):
        return _dev.xg_vecplace_dispatches(self._v)

    @property
    def views(self):
        """the views of more than one row (0 unless loaded with views=True)"""
        return _dev.xg_vecplace_views(self._v)

    def close(self):
        if getattr(self, "_v", None):
            _check(_dev.xg_vecplace_free(self._v), "xg_vecplace_free")
            self._v = None
        if getattr(self, "regions", None):
            self.regions.close()
            self.regions = None


def vec_check(run, batch=65536):
    """A VecPlace after its run: xg_chk_spans of every block of every row on both sides of the
    placement, at most `batch` spans a launch.  Returns the list indices (vec_index) of the rows with
    a differing block, ascending."""
    bad, src, dst, who = set(), [], [], []

    def flush():
        a, b = chk_spans(run, src), chk_spans(run, dst)
        bad.update(k for k, x, y in zip(who, a, b) if x != y)
        del src[:], dst[:], who[:]
    for k, r in enumerate(run.rows):
        for j in range(r.count):
            src.append((r.src_buf, r.src_off + j * r.src_step, r.len))
            dst.append((r.dst_buf, r.dst_off + j * r.dst_step, r.len))
            who.append(k)
            if len(who) == batch:
                flush()
    if who:
        flush()
    return sorted(run.vec_index[k] for k in bad)


class MethodRun:
    """prepare_*_data + the compiled plan of one method on this GPU:
    HBM regions, fingerprint fill (untimed), plan upload.  regions: a Regions
    object to use (re-poisoned here, not freed by close()) instead of new ones.
    fill=False: SEND keeps what it holds (a caller's payload, written with write() or adopted
    with Regions.adopt); check delivery with payload_check()."""

    def __init__(self, ctx, sched, it=0, mode=0, pack_max_seg=4 << 20, regions=None, pack_min=0, pack_form=-1,
                 fill=True):
        d = device()
        if fill and sched.ragged:
            raise XGError("MethodRun: the fingerprint fill takes no ragged schedule (segments of one length "
                          "only): pass fill=False, write the payload, and check it with payload_check()")
        self.ctx, self.sched, self.it, self.mode, self.pack_max_seg = ctx, sched, it, mode, pack_max_seg
        self.pack_min, self.pack_form = pack_min, pack_form
        G, g = ctx.nranks, ctx.rank
        if G > 1 and not getattr(ctx, "is_virtual", False):
            # a real multi-GPU job: refuse, on every rank alike, calls RCCL would not pair
            # step by step, before any rank posts one (xg_devplans_match)
            sched.check_pairing(G, pack_max_seg, pack_min, pack_form, d.xg_self_max(ctx.handle))
        self.view = sched.devplan(G, g, pack_max_seg, pack_min, pack_form)
        self._shared = regions is not None
        if regions is not None:
            if not regions.fits(self.view.region_bytes):
                raise XGError("MethodRun: shared regions too small for this plan")
            self._r = regions._r
            _check(d.xg_regions_poison(self._r), "xg_regions_poison")
        else:
            rb = (C.c_int64 * NBUF)(*self.view.region_bytes)
            self._r = C.c_void_p()
            _check(d.xg_regions_alloc(ctx.handle, rb, C.byref(self._r)), "xg_regions_alloc")
        n = host().xg_fill_runs(sched.handle, G, g, None)
        runs = (SegRun * max(1, n))()
        host().xg_fill_runs(sched.handle, G, g, runs)
        if fill:
            _check(d.xg_fill(self._r, runs, n, sched.d, it, mode), "xg_fill")
        ns = host().xg_verify_slots(sched.handle, G, g, None)
        self._slots = (Slot * max(1, ns))()
        host().xg_verify_slots(sched.handle, G, g, self._slots)
        self.nslots = ns
        self.slots = [(s.src, s.seed, s.dst, s.off) for s in self._slots[:ns]]
        self._p = C.c_void_p()
        _check(d.xg_plan_load(ctx.handle, self._r, self.view.ptr, C.byref(self._p)), "xg_plan_load")
        self.nsteps = d.xg_plan_nsteps(self._p)
        self.set_step_marks(sched.timed_steps())       # as xg_run_method: only the steps a Timer reads
        self.engine_workgroups = d.xg_plan_engine(self._p)   # 0: one launch per step
        self.engine_rails = d.xg_plan_engine_rails(self._p)  # > 0: a solo segment on that many rails

    def run_timed(self):
        """barrier-free timed run; returns (step_done[], step_post[], wall)."""
        n = max(1, self.nsteps)
        done, post, wall = (C.c_double * n)(), (C.c_double * n)(), C.c_double()
        _check(_dev.xg_plan_run(self._p, done, post, C.byref(wall)), "xg_plan_run")
        return list(done)[:self.nsteps], list(post)[:self.nsteps], wall.value

    def enqueue(self):
        _check(_dev.xg_plan_enqueue(self._p), "xg_plan_enqueue")

    def check(self):
        """after a synchronised enqueue(): raise if a step-engine barrier timed out"""
        _check(_dev.xg_plan_check(self._p), "xg_plan_check")

    @property
    def launches(self):
        """kernel launches per run (copy + engine launches)"""
        return _dev.xg_plan_launches(self._p)

    def engine_steps(self):
        """(steps inside engine segments, segments, hazard barriers)"""
        ns, nh = C.c_int(), C.c_int()
        n = _dev.xg_plan_engine_steps(self._p, C.byref(ns), C.byref(nh))
        return n, ns.value, nh.value

    def wave_launches(self):
        """(copy launches that run copy_kernel_w, the context's wave grid, most pieces on one wave)"""
        return plan_wave_launches(self._p)

    def shift_launches(self):
        """copy launches that run copy_kernel_s, the shifted piece copy (xg_plan_shift_launches)"""
        return _dev.xg_plan_shift_launches(self._p)

    def extent_launches(self):
        """copy launches that run copy_kernel_x, the extent copy (xg_plan_extent_launches)"""
        return _dev.xg_plan_extent_launches(self._p)

    def displs(self):
        """staging displacements of the packed segments, as the device scan computed them"""
        n = _dev.xg_plan_displs(self._p, None, 0)
        out = (C.c_int64 * max(1, n))()
        _check(_dev.xg_plan_displs(self._p, out, n), "xg_plan_displs")
        return list(out)[:n]

    def write(self, buf, off, data):
        """test hook: overwrite bytes of a region"""
        b = C.create_string_buffer(bytes(data), len(data))
        _check(_dev.xg_regions_write(self._r, buf, off, b, len(data)), "xg_regions_write")

    def poison(self):
        _check(_dev.xg_regions_poison(self._r), "xg_regions_poison")

    def set_step_marks(self, need=None):
        """mark only the steps with need[s] set in a timed run (None: every step), the others
        reported as done with the next marked one (xg_plan_set_step_marks)"""
        arr = (C.c_uint8 * max(1, self.nsteps))(*need) if need is not None else None
        _check(_dev.xg_plan_set_step_marks(self._p, arr), "xg_plan_set_step_marks")

    def set_local_only(self, on=True):
        """test hook (virtual GPU): run this GPU's share alone -- copy launches only, its RCCL
        calls and in-loop barriers left out (xg_plan_set_local_only)"""
        _check(_dev.xg_plan_set_local_only(self._p, 1 if on else 0), "xg_plan_set_local_only")

    def engine_preset(self, tickets=0, armed=0):
        """test hook: the engine counters as earlier launches would have left them -- `tickets`
        grid tickets, `armed` armed solo launches (xg_plan_engine_preset)"""
        _check(_dev.xg_plan_engine_preset(self._p, tickets & 0xFFFFFFFF, armed & 0xFFFFFFFF), "xg_plan_engine_preset")

    def verify(self):
        ns = max(1, self.nslots)
        chk, bad, first = (C.c_uint64 * ns)(), (C.c_int64 * ns)(), (C.c_int64 * ns)()
        _check(_dev.xg_verify(self._r, self._slots, self.nslots, self.sched.d, self.it, self.mode,
                              chk, bad, first), "xg_verify")
        return list(chk)[:self.nslots], list(bad)[:self.nslots], list(first)[:self.nslots]

    def slot_chk(self):
        """xg_chk64 of every receive slot (self.slots order) by xg_chk_spans -- no fingerprint
        needed; equals verify()[0]"""
        G, g = self.ctx.nranks, self.ctx.rank
        ln = [n for q, n in zip(self.sched.deliveries(G), self.sched.delivery_lens(G)) if q.dst_gpu == g]
        return chk_spans(self, [(BUF_RECV, off, n) for (_s, _e, _d, off), n in zip(self.slots, ln)])

    def read(self, buf, off, length):
        out = C.create_string_buffer(max(1, length))
        _check(_dev.xg_regions_read(self._r, buf, off, out, length), "xg_regions_read")
        return out.raw[:length]

    def close(self):
        if getattr(self, "_p", None):
            _check(_dev.xg_plan_free(self._p), "xg_plan_free")
            self._p = None
        if getattr(self, "_r", None):
            if not self._shared:
                _check(_dev.xg_regions_free(self._r), "xg_regions_free")
            self._r = None
