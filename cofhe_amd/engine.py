"""ctypes loader of libcofhe_hip.so (C ABI: include/cofhe_hip.h)."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

REC_WORDS = 168
EXP_REC_WORDS = 32

COFHE_HIP_EINVAL, COFHE_HIP_ESHAPE, COFHE_HIP_ENDIM, COFHE_HIP_EHIP, COFHE_HIP_ENOMEM = -1, -2, -3, -4, -5

# Every prototype of include/cofhe_hip.h as "return:parameters", one letter each (tests/test_engine_signatures_cpu.py compares the
# table with the header).  Parameters: p pointer (anything with * or []), u uint32_t, q uint64_t, z size_t, i int, l int64_t.
# Returns: i int, v void, z size_t, s const char *.
_CTYPES = {"p": C.c_void_p, "u": C.c_uint32, "q": C.c_uint64, "z": C.c_size_t, "i": C.c_int, "l": C.c_int64, "v": None, "s": C.c_char_p}
SIGNATURES = {
    "cofhe_hip_last_error": "s:",
    "cofhe_hip_record_words": "i:",
    "cofhe_hip_exp_words": "i:",
    "cofhe_hip_ctx_create": "i:ipzp",
    "cofhe_hip_ctx_destroy": "v:p",
    "cofhe_hip_malloc": "i:pzp",
    "cofhe_hip_free": "i:pp",
    "cofhe_hip_free_on_stream": "i:ppp",
    "cofhe_hip_trim": "i:pz",
    "cofhe_hip_ctx_set_option": "i:ppl",
    "cofhe_hip_profile_read": "i:ppppi",
    "cofhe_hip_upload": "i:pppzp",
    "cofhe_hip_download": "i:pppzp",
    "cofhe_hip_stream_sync": "i:pp",
    "cofhe_hip_stream_create": "i:pip",
    "cofhe_hip_stream_destroy": "i:pp",
    "cofhe_hip_stream_query": "i:ppp",
    "cofhe_hip_device_status": "i:ppip",
    "cofhe_hip_validate_records": "i:ppqpp",
    "cofhe_hip_compose_records": "i:ppppqp",
    "cofhe_hip_compose_wide_records": "i:ppppqupp",
    "cofhe_hip_add_ciphertext_records": "i:ppppqp",
    "cofhe_hip_sub_ciphertext_records": "i:ppppqp",
    "cofhe_hip_invert_records": "i:pppqp",
    "cofhe_hip_pow_records": "i:ppppqp",
    "cofhe_hip_scal_matmul_records": "i:pppppuuup",
    "cofhe_hip_matmul_plain_ct_records": "i:pppppuuup",
    "cofhe_hip_conv2d_out_shape": "i:ppp",
    "cofhe_hip_conv2d_plain_ct_records": "i:ppppppp",
    "cofhe_hip_conv2d_geometry_out_shape": "i:ppp",
    "cofhe_hip_conv2d_grouped_plain_ct_records": "i:ppppppp",
    "cofhe_hip_sum_pool2d_records": "i:pppppp",
    "cofhe_hip_matmul_plain_plain_records": "i:ppppuuuup",
    "cofhe_hip_conv2d_plain_plain_records": "i:pppppup",
    "cofhe_hip_conv2d_ct_filters_records": "i:ppppppp",
    "cofhe_hip_pow_dot_records": "i:ppppqup",
    "cofhe_hip_poly_shift_records": "i:ppppquup",
    "cofhe_hip_poly_close_records": "i:ppppppquup",
    "cofhe_hip_divfloor_plain_records": "i:pppqpqup",
    "cofhe_hip_div_close_records": "i:pppqpppqup",
    "cofhe_hip_divmod_plain_records": "i:pppqppquup",
    "cofhe_hip_divx_rows_records": "i:pppqpquup",
    "cofhe_hip_divx_tuples_records": "i:pppqpppppquup",
    "cofhe_hip_divx_close_records": "i:pppqpuppqup",
    "cofhe_hip_divx_shape": "i:upupp",
    "cofhe_hip_lut_rotate_records": "i:ppqppqup",
    "cofhe_hip_lut_tuples_records": "i:ppqppppppquup",
    "cofhe_hip_lut_select_records": "i:ppppqup",
    "cofhe_hip_lut_tuples_shape_bits": "i:upupp",
    "cofhe_hip_cmp_rows_records": "i:pppquuup",
    "cofhe_hip_cmp_tuples_records": "i:pppppppquuup",
    "cofhe_hip_cmp_close_records": "i:pppppquuup",
    "cofhe_hip_cmp_shape": "i:uuuupuppp",
    "cofhe_hip_view_check": "i:ppppp",
    "cofhe_hip_view_permute": "i:pupp",
    "cofhe_hip_view_slice": "i:pupppp",
    "cofhe_hip_view_pad": "i:puppp",
    "cofhe_hip_view_broadcast": "i:pupup",
    "cofhe_hip_view_window_taps": "i:pp",
    "cofhe_hip_view_into": "i:ppp",
    "cofhe_hip_view_records": "i:pppppup",
    "cofhe_hip_gather_records": "i:ppqpppqup",
    "cofhe_hip_spline_rows_records": "i:ppqppquuuup",
    "cofhe_hip_spline_tuples_records": "i:ppqppppppquuuup",
    "cofhe_hip_spline_powers_records": "i:pppquup",
    "cofhe_hip_spline_close_records": "i:ppppquuuup",
    "cofhe_hip_spline_tuples_shape": "i:upuppp",
    "cofhe_hip_decrypt_records": "i:pppppqup",
    "cofhe_hip_accumulate_records": "i:ppppuuup",
    "cofhe_hip_pow_form_records": "i:ppppqp",
    "cofhe_hip_pow_fixed_base_record": "i:ppppp",
    "cofhe_hip_pow_fixed_base_records": "i:pupppp",
    "cofhe_hip_encrypt_records": "i:pppppqup",
    "cofhe_hip_pow_fixed_base_many_records": "i:ppppqp",
    "cofhe_hip_encrypt_fresh_records": "i:pppppppqup",
    "cofhe_hip_rerandomize_records": "i:ppppppqp",
    "cofhe_hip_add_plain_records": "i:ppppppppquip",
    "cofhe_hip_comb_shape": "i:uquuuqppp",
    "cofhe_hip_part_decrypt_records": "i:ppppqp",
    "cofhe_hip_combine_part_decryptions_records": "i:pppupppqup",
    "cofhe_hip_time_compose": "i:ppppqipp",
    "cofhe_hip_workspace_plan": "i:ppupupp",
    "cofhe_hip_timer_start": "i:ppp",
    "cofhe_hip_timer_stop": "i:pppp",
    "cofhe_hip_bytes_to_records": "i:pzpppp",
    "cofhe_hip_records_to_bytes": "i:pquppp",
    "cofhe_hip_pdr_bytes_to_records": "i:pzpppp",
    "cofhe_hip_pdr_records_to_bytes": "i:pquppp",
    "cofhe_hip_unpack_tensor_device": "i:ppzipqpppp",
    "cofhe_hip_pack_tensor_device": "i:ppqiuppzpp",
    "cofhe_hip_packed_size_bound": "z:qiu",
    "cofhe_hip_bytes_to_exponents": "i:pzpppp",
    "cofhe_hip_host_free": "v:p",
    "cofhe_hip_add_ciphertext_tensors_bytes": "i:ppzpzpp",
    "cofhe_hip_sub_ciphertext_tensors_bytes": "i:ppzpzpp",
    "cofhe_hip_add_plaintext_tensor_bytes": "i:ppzpzpuipp",
    "cofhe_hip_matmul_plain_ct_tensors_bytes": "i:ppzpzpzpp",
    "cofhe_hip_conv2d_plain_ct_tensors_bytes": "i:ppzpzpzuuuupp",
    "cofhe_hip_conv2d_grouped_plain_ct_tensors_bytes": "i:ppzpzpzuuuuuuupp",
    "cofhe_hip_sum_pool2d_tensors_bytes": "i:ppzpzuuuuuupp",
    "cofhe_hip_poly_close_tensors_bytes": "i:ppzpzpzpupp",
    "cofhe_hip_div_close_tensors_bytes": "i:ppzpzpzpupp",
    "cofhe_hip_scal_ciphertext_tensors_bytes": "i:ppzpzpzpp",
    "cofhe_hip_shard_rows": "v:quupp",
    "cofhe_hip_comm_unique_id": "i:p",
    "cofhe_hip_comm_create": "i:ppuup",
    "cofhe_hip_comm_destroy": "v:p",
    "cofhe_hip_all_gather_rows": "i:pppqqpp",
    "cofhe_hip_gather_plan": "i:qquppp",
    "cofhe_hip_comm_info": "i:pppp",
    "cofhe_hip_comm_set_option": "i:ppl",
}


class CofheHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("cofhe_hip error %d: %s" % (code, msg))
        self.code = code
        self.message = msg


def lib_path():
    return os.path.join(_HERE, "libcofhe_hip.so")


def load_library(path=None):
    """Loads the HIP extension; raises when it has not been built (no fallback exists).  `path`: another build of the
    SAME extension (tools/build_variant.sh; bench.py --lib), honoured by the first call only."""
    global _LIB
    if _LIB is None:
        p = path or lib_path()
        if not os.path.exists(p):
            raise FileNotFoundError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % p)
        # A process that also uses PyTorch holds two HIP runtimes (the wheel bundles its own libamdhip64.so, this
        # library binds /opt/rocm's libamdhip64.so.7), and the pair only works when PyTorch's has initialised the
        # device first.  If the host application has already imported torch, do that here.
        import sys
        torch = sys.modules.get("torch")
        if torch is not None:
            try:
                if torch.cuda.is_available() and not torch.cuda.is_initialized():
                    torch.cuda.init()
            except Exception:       # a CPU-only torch build: nothing to order
                pass
        L = C.CDLL(p)
        for name, sig in SIGNATURES.items():
            fn = getattr(L, name, None)
            if fn is None:
                raise AttributeError("%s does not export %s: a build older than include/cofhe_hip.h" % (p, name))
            ret, params = sig.split(":")
            fn.restype = _CTYPES[ret]
            fn.argtypes = [_CTYPES[c] for c in params]
        _LIB = L
    return _LIB


def _chk(rc):
    if rc != 0:
        raise CofheHipError(rc, load_library().cofhe_hip_last_error().decode())


def _absdelta(delta):
    assert delta < 0
    m = -delta
    return m.to_bytes((m.bit_length() + 7) // 8, "little")


def _host_record(x, words=REC_WORDS):
    """a host record argument (f_record, h_record, pk_record, base_record; words=EXP_REC_WORDS: an exponent record) as a
    contiguous uint32 array of exactly `words` words -- the library reads that many.  Pass its .ctypes.data and keep the array
    in a local for the length of the call."""
    import numpy as np
    a = np.ascontiguousarray(x, dtype=np.uint32)
    assert a.size == words
    return a


def _u32s(values):
    """a uint32_t shape array argument (never of length 0: the count travels beside it)"""
    return (C.c_uint32 * max(1, len(values)))(*values)


class _DeviceScope:
    """the device allocations of one Engine call on serialised tensors, freed on the way out (also by an exception): how the
    entries that the library has no entry point for go from bytes to records, through a launcher and back to bytes"""

    def __init__(self, eng):
        self.eng = eng
        self.held = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.held:
            self.eng.free(p)

    def alloc(self, nbytes):
        p = self.eng.malloc(nbytes)
        self.held.append(p)
        return p

    def load(self, t, kind):
        """serialised tensor -> (d_records, shape, n_records); unpack_tensor_device validates the incoming forms"""
        # every integer owns an 8-byte table entry: the record count is bounded by the length
        cap = (len(t) // 8) // (3 if kind else 1) + 1
        raw = self.alloc(len(t) + 4)
        recs = self.alloc(cap * 4 * (REC_WORDS if kind else EXP_REC_WORDS))
        self.eng.upload(raw, t)
        shape, n = self.eng.unpack_tensor_device(raw, len(t), kind, recs, cap)
        return recs, shape, n

    def packed(self, d_records, n_records, kind, shape):
        """records on the device -> the serialised tensor, as bytes"""
        cap = self.eng.packed_size_bound(n_records, kind, len(shape))
        buf = self.alloc(cap)
        ln = self.eng.pack_tensor_device(d_records, n_records, kind, shape, buf, cap)
        return self.eng.download(buf, ln, dtype="uint8").tobytes()


class Engine:
    """One GPU + one discriminant.  All tensors cross as bytes in the reference's binary
    formats (or as device pointers to records for the resident-tensor entry points)."""

    def __init__(self, delta: int, device: int = 0):
        self.L = load_library()
        self.ctx = C.c_void_p()
        d = _absdelta(delta)
        _chk(self.L.cofhe_hip_ctx_create(device, d, len(d), C.byref(self.ctx)))
        self.delta = delta
        self.device = device

    def close(self):
        if self.ctx:
            self.L.cofhe_hip_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, fn, *args):
        """fn(ctx, *args), then the error check: integers as integers and device pointers, bytes as host buffers"""
        _chk(fn(self.ctx, *args))

    # ---- whole ops on host byte buffers -------------------------------------------------
    def _take(self, out, outlen):
        data = C.string_at(out, outlen.value)
        self.L.cofhe_hip_host_free(out)
        return data

    def _bytes_out(self, fn, *args):
        """fn(*args, uint8_t **out, size_t *outlen): the bytes the library allocated, which it gets back"""
        out, n = C.c_void_p(), C.c_size_t()
        _chk(fn(*args, C.byref(out), C.byref(n)))
        return self._take(out, n)

    def add_ciphertext_tensors(self, t1: bytes, t2: bytes) -> bytes:
        return self._bytes_out(self.L.cofhe_hip_add_ciphertext_tensors_bytes, self.ctx, t1, len(t1), t2, len(t2))

    def sub_ciphertext_tensors(self, t1: bytes, t2: bytes) -> bytes:
        """t1 - t2 element-wise (the compute node's SUBTRACT): one composition per record, with the inverse of t2's forms"""
        return self._bytes_out(self.L.cofhe_hip_sub_ciphertext_tensors_bytes, self.ctx, t1, len(t1), t2, len(t2))

    def add_plaintext_tensor(self, cts: bytes, pt: bytes, f_record, kbits: int, mode: int = 0) -> bytes:
        """mode 0: cts + pt, 1: cts - pt, 2: pt - cts, without an encryption: (c1, c2 o f^m); f_record: host uint32[168]"""
        f = _host_record(f_record)
        return self._bytes_out(self.L.cofhe_hip_add_plaintext_tensor_bytes, self.ctx, cts, len(cts), pt, len(pt), f.ctypes.data, kbits, mode)

    def poly_close_tensors(self, coef: bytes, e: bytes, powers: bytes, f_record, kbits: int) -> bytes:
        """coef (plaintext tensor [d + 1]), e (plaintext tensor of the opened values x - a) and powers (ciphertext tensor
        [d, shape of e] of the power tuples [a^i]) -> the ciphertext tensor of p(x), of e's shape; f_record: host uint32[168]"""
        f = _host_record(f_record)
        return self._bytes_out(self.L.cofhe_hip_poly_close_tensors_bytes, self.ctx, coef, len(coef), e, len(e), powers, len(powers),
                               f.ctypes.data, kbits)

    def div_close_tensors_bytes(self, e: bytes, div: bytes, rq: bytes, f_record, kbits: int) -> bytes:
        """e (plaintext tensor of the opened values x - r), div (plaintext tensor of one divisor, of e's last dimension or of e's
        shape) and rq (ciphertext tensor [r_q] of e's shape) -> the ciphertext tensor of floor(x / div) or one less, of e's
        shape; a divisor outside [1, 2^(kbits-1)) is refused; f_record: host uint32[168]"""
        f = _host_record(f_record)
        return self._bytes_out(self.L.cofhe_hip_div_close_tensors_bytes, self.ctx, e, len(e), div, len(div), rq, len(rq),
                               f.ctypes.data, kbits)

    def divx_close_tensors_bytes(self, e: bytes, div: bytes, tuples: bytes, f_record, kbits: int) -> bytes:
        """e (plaintext tensor of the opened values x - r, shape S, at most 7 dimensions), div (plaintext tensor of one divisor, of
        e's last dimension or of e's shape) and tuples (ciphertext tensor of the exact-division tuples' entries, shape S + [rows],
        1 <= rows <= 4096) -> the ciphertext tensor of floor(x / div), shape S; f_record: host uint32[168].  Composed here from
        unpack_tensor_device (which validates the incoming forms), divx_shape (COFHE_HIP_ESHAPE when the tuples' shape is anything
        else, as for a divisor tensor of another shape), divx_close_records and pack_tensor_device, exactly as
        lut_select_tensors_bytes is: the library has no entry point of its own for it."""
        with _DeviceScope(self) as dev:
            de, se, ne = dev.load(e, 0)
            dd, sd, nd = dev.load(div, 0)
            dt, st, nt = dev.load(tuples, 2)
            rows = self.divx_shape(se, st)
            if list(sd) not in ([1], list(se[-1:]), list(se)):
                raise CofheHipError(-2, "divx_close: the divisors are one element, e's last dimension or e's shape")
            assert nt == 2 * ne * rows                                # the counts are the shapes' products
            dout = dev.alloc(max(ne, 1) * 2 * REC_WORDS * 4)
            self.divx_close_records(de, dd, nd, dt, rows, f_record, dout, ne, kbits)
            return dev.packed(dout, 2 * ne, 2, se)

    def lut_select_tensors_bytes(self, e: bytes, tuples: bytes) -> bytes:
        """e (plaintext tensor of the opened values x - r, shape S, at most 7 dimensions) and tuples (ciphertext tensor of the
        lookup tuples' entries, shape S + [2^bits], 1 <= bits <= 12) -> the ciphertext tensor of the entries e mod 2^bits, shape S.
        Composed here from unpack_tensor_device (which validates the incoming forms), lut_tuples_shape_bits (COFHE_HIP_ESHAPE when
        the tuples' shape is anything else), lut_select_records and pack_tensor_device: the library has no entry point of its own
        for it."""
        with _DeviceScope(self) as dev:
            de, se, ne = dev.load(e, 0)
            dt, st, nt = dev.load(tuples, 2)
            bits = self.lut_tuples_shape_bits(se, st)
            assert nt == 2 * (ne << bits)                             # the counts are the shapes' products
            dout = dev.alloc(max(ne, 1) * 2 * REC_WORDS * 4)
            self.lut_select_records(de, dt, dout, ne, bits)
            return dev.packed(dout, 2 * ne, 2, se)

    def spline_close_tensors_bytes(self, e: bytes, tuples: bytes, shift: int, kbits: int) -> bytes:
        """e (plaintext tensor of the opened values x - r, shape S, at most 6 dimensions) and tuples (ciphertext tensor of the spline
        tuples' entries, shape S + [2^bits, d + 1]) -> the ciphertext tensor of the spline's values, shape S; shift: the segment-width
        bits of the table.  Composed here from unpack_tensor_device (which validates the incoming forms), spline_tuples_shape
        (COFHE_HIP_ESHAPE when the tuples' shape is anything else), spline_close_records and pack_tensor_device, exactly as
        lut_select_tensors_bytes is: the library has no entry point of its own for it."""
        with _DeviceScope(self) as dev:
            de, se, ne = dev.load(e, 0)
            dt, st, nt = dev.load(tuples, 2)
            bits, d = self.spline_tuples_shape(se, st)
            assert nt == 2 * (ne << bits) * (d + 1)                   # the counts are the shapes' products
            dout = dev.alloc(max(ne, 1) * 2 * REC_WORDS * 4)
            self.spline_close_records(de, dt, dout, ne, bits, shift, d, kbits)
            return dev.packed(dout, 2 * ne, 2, se)

    def cmp_close_tensors_bytes(self, e: bytes, tuples: bytes, bits: int, digit_bits: int, kbits: int):
        """e (plaintext tensor of the opened values x - r, shape S, at most 6 dimensions) and tuples (ciphertext tensor of the
        comparison tuples' entries, shape S + [nd, 2^digit_bits], nd = ceil(bits / digit_bits)) -> (the ciphertext tensor of the
        pairs [S_A], [S_B], shape S + [2], the plaintext tensor wrap of shape S).  Composed here from unpack_tensor_device (which
        validates the incoming forms), cmp_shape (COFHE_HIP_ESHAPE when the tuples' shape is anything else), cmp_close_records
        and pack_tensor_device, exactly as lut_select_tensors_bytes is: the library has no entry point of its own for it."""
        with _DeviceScope(self) as dev:
            de, se, ne = dev.load(e, 0)
            dt, st, nt = dev.load(tuples, 2)
            _, entries = self.cmp_shape(bits, digit_bits, kbits, se, st)
            assert nt == 2 * ne * entries                              # the counts are the shapes' products
            dout = dev.alloc(max(ne, 1) * 4 * REC_WORDS * 4)
            dwrap = dev.alloc(max(ne, 1) * EXP_REC_WORDS * 4)
            self.cmp_close_records(de, dt, dout, dwrap, ne, bits, digit_bits, kbits)
            return dev.packed(dout, 4 * ne, 2, se + [2]), dev.packed(dwrap, ne, 0, se)

    def scal_ciphertext_tensors(self, s: bytes, cts: bytes, zero: bytes = None) -> bytes:
        return self._bytes_out(self.L.cofhe_hip_scal_ciphertext_tensors_bytes, self.ctx, s, len(s), cts, len(cts),
                               zero, len(zero) if zero else 0)

    def matmul_plain_ct_tensors(self, s: bytes, cts: bytes, zero: bytes) -> bytes:
        """s (plaintext tensor, n x m) . cts (ciphertext tensor, m x p) from zero (1-element ciphertext tensor): the linear
        layer y = W x with plaintext weights, the mirror image of the 2-D scal_ciphertext_tensors"""
        return self._bytes_out(self.L.cofhe_hip_matmul_plain_ct_tensors_bytes, self.ctx, s, len(s), cts, len(cts), zero, len(zero))

    def conv2d_plain_ct_tensors(self, w: bytes, cts: bytes, zero: bytes, stride=(1, 1), pad=(0, 0), dilation=(1, 1), groups=1) -> bytes:
        """w (plaintext tensor [kh, kw, C / groups, Co]) over cts (ciphertext tensor [B, H, W, C]), channels last, from zero
        (1-element ciphertext tensor); stride, zero padding and dilation as (rows, columns).  Returns the ciphertext tensor
        [B, Ho, Wo, Co]"""
        head = (self.ctx, w, len(w), cts, len(cts), zero, len(zero), stride[0], stride[1], pad[0], pad[1])
        if tuple(dilation) == (1, 1) and groups == 1:
            return self._bytes_out(self.L.cofhe_hip_conv2d_plain_ct_tensors_bytes, *head)
        return self._bytes_out(self.L.cofhe_hip_conv2d_grouped_plain_ct_tensors_bytes, *head, dilation[0], dilation[1], groups)

    def conv2d_ct_filters_tensors(self, img: bytes, filters: bytes, zero: bytes, stride=(1, 1), pad=(0, 0), dilation=(1, 1)) -> bytes:
        """the plaintext tensor img [B, H, W, C] under the ciphertext tensor filters [kh, kw, C, Co], channels last, from zero
        (1-element ciphertext tensor); stride, zero padding and dilation as (rows, columns).  Returns the ciphertext tensor
        [B, Ho, Wo, Co]: the E * [Bf] term of a convolution Beaver triplet.  Composed here from unpack_tensor_device (which
        validates the incoming forms), conv2d_ct_filters_records and pack_tensor_device, as lut_select_tensors_bytes is: the
        library has no entry point of its own for it.  COFHE_HIP_ESHAPE when an operand is not 4-D or the channels differ"""
        with _DeviceScope(self) as dev:
            di, si, _ = dev.load(img, 0)
            df, sf, _ = dev.load(filters, 2)
            if len(si) != 4 or len(sf) != 4:
                raise CofheHipError(COFHE_HIP_ESHAPE, "conv2d_ct_filters takes a 4-D image tensor [B, H, W, C] and a 4-D filter tensor [kh, kw, C, Co]")
            ho, wo = conv2d_out_shape(si, sf, stride, pad, dilation, 1)          # ESHAPE when the channels differ
            dz, _, nz = dev.load(zero, 2)
            if nz != 2:
                raise CofheHipError(COFHE_HIP_EINVAL, "zero must be a one-element ciphertext tensor")
            so = [si[0], ho, wo, sf[3]]
            nout = 2 * so[0] * ho * wo * so[3]
            dout = dev.alloc(max(nout, 1) * REC_WORDS * 4)
            self.conv2d_ct_filters_records(di, df, dz, dout, si, sf, stride, pad, dilation=dilation)
            return dev.packed(dout, nout, 2, so)

    def sum_pool2d_tensors(self, cts: bytes, zero: bytes, kernel, stride=None, pad=(0, 0)) -> bytes:
        """the sums over kernel = (kh, kw) windows of the ciphertext tensor cts [B, H, W, C], channel by channel, from zero;
        stride defaults to the kernel.  Returns [B, Ho, Wo, C].  Average pooling: fold 1 / (kh kw) into the next layer's weights"""
        stride = kernel if stride is None else stride
        return self._bytes_out(self.L.cofhe_hip_sum_pool2d_tensors_bytes, self.ctx, cts, len(cts), zero, len(zero),
                               kernel[0], kernel[1], stride[0], stride[1], pad[0], pad[1])

    # ---- format conversion (host) ----------------------------------------------------------
    def _to_records(self, fn, t, words):
        """fn: a bytes -> (shape, records of `words` words) converter of the library, which gets its array back"""
        import numpy as np
        ndim, shape, recs, n = C.c_uint32(), (C.c_uint32 * 8)(), C.POINTER(C.c_uint32)(), C.c_uint64()
        _chk(fn(t, len(t), C.byref(ndim), shape, C.byref(recs), C.byref(n)))
        arr = np.ctypeslib.as_array(recs, shape=(n.value * words,)).copy() if n.value else np.zeros(0, dtype=np.uint32)
        self.L.cofhe_hip_host_free(recs)
        return list(shape[:ndim.value]), arr

    def _from_records(self, fn, recs, shape, words):
        """fn: a (records of `words` words, shape) -> bytes converter of the library"""
        import numpy as np
        recs = np.ascontiguousarray(recs, dtype=np.uint32)
        return self._bytes_out(fn, recs.ctypes.data, recs.size // words, len(shape), _u32s(shape))

    def bytes_to_records(self, t: bytes):
        return self._to_records(self.L.cofhe_hip_bytes_to_records, t, REC_WORDS)

    def records_to_bytes(self, recs, shape) -> bytes:
        return self._from_records(self.L.cofhe_hip_records_to_bytes, recs, shape, REC_WORDS)

    def pdr_bytes_to_records(self, t: bytes):
        """partial-decryption tensor (one form per element) -> records"""
        return self._to_records(self.L.cofhe_hip_pdr_bytes_to_records, t, REC_WORDS)

    def pdr_records_to_bytes(self, recs, shape) -> bytes:
        return self._from_records(self.L.cofhe_hip_pdr_records_to_bytes, recs, shape, REC_WORDS)

    def bytes_to_exponents(self, t: bytes):
        return self._to_records(self.L.cofhe_hip_bytes_to_exponents, t, EXP_REC_WORDS)

    # ---- format conversion on the GPU (device pointers) ------------------------------------
    def unpack_tensor_device(self, d_bytes, nbytes, kind, d_records, capacity_records, stream=0):
        """kind 2 ciphertexts / 1 partial decryptions / 0 plaintexts; returns (shape, n_records)"""
        ndim, shape, n = C.c_uint32(), (C.c_uint32 * 8)(), C.c_uint64()
        self._call(self.L.cofhe_hip_unpack_tensor_device, d_bytes, nbytes, kind, d_records, capacity_records, C.byref(ndim), shape,
                   C.byref(n), stream)
        return list(shape[:ndim.value]), n.value

    def pack_tensor_device(self, d_records, n_records, kind, shape, d_bytes, capacity, stream=0) -> int:
        """returns the serialised length written to d_bytes"""
        n = C.c_size_t()
        self._call(self.L.cofhe_hip_pack_tensor_device, d_records, n_records, kind, len(shape), _u32s(shape), d_bytes, capacity,
                   C.byref(n), stream)
        return n.value

    def packed_size_bound(self, n_records, kind, ndim) -> int:
        return self.L.cofhe_hip_packed_size_bound(n_records, kind, ndim)

    # ---- kernels on device-resident records (pointers are ints, e.g. torch .data_ptr()) -----
    def compose_records(self, d_a, d_b, d_out, n_records, stream=0):
        self._call(self.L.cofhe_hip_compose_records, d_a, d_b, d_out, n_records, stream)

    def compose_wide_records(self, d_a, d_b, d_out, n_records, reps=1, count_fallbacks=False, stream=0):
        """one composition per wavefront in the wavefront-wide layout (the latency kernels' composition); returns the number
        of pairs that took the 8-lane fallback when count_fallbacks"""
        fb = C.c_uint32(0)
        self._call(self.L.cofhe_hip_compose_wide_records, d_a, d_b, d_out, n_records, reps, C.byref(fb) if count_fallbacks else None, stream)
        return int(fb.value)

    def add_ciphertext_records(self, d_a, d_b, d_out, n_ciphertexts, stream=0):
        """ciphertext-level add: folds the shared c1 of encrypt_tensor-made operands (n + 1 compositions, not 2 n)"""
        self._call(self.L.cofhe_hip_add_ciphertext_records, d_a, d_b, d_out, n_ciphertexts, stream)

    def sub_ciphertext_records(self, d_a, d_b, d_out, n_ciphertexts, stream=0):
        """out[i] = a[i] - b[i]: a o b^-1 per record, folding and launch routes as add_ciphertext_records; d_out may be d_a or d_b"""
        self._call(self.L.cofhe_hip_sub_ciphertext_records, d_a, d_b, d_out, n_ciphertexts, stream)

    def invert_records(self, d_in, d_out, n_records, stream=0):
        """out[i] = in[i]^-1 on form records (a ciphertext tensor: Enc(-m) at no composition); in place allowed"""
        self._call(self.L.cofhe_hip_invert_records, d_in, d_out, n_records, stream)

    def add_plain_records(self, d_cts, d_plain, f_record, d_out, n_ciphertexts, kbits, mode=0, d_r=None, h_record=None, pk_record=None,
                          stream=0):
        """mode 0: ct + m, 1: ct - m, 2: m - ct (d_plain: n exponent records).  Without d_r: (c1, c2 o f^m), deterministic and
        purely stream-ordered; with d_r (n exponent records) and the host records h, pk: fresh randomness in the same tree.
        d_out may be d_cts."""
        f = _host_record(f_record)
        hp = [_host_record(h_record), _host_record(pk_record)] if d_r is not None else []
        self._call(self.L.cofhe_hip_add_plain_records, d_cts, d_plain, d_r, *([x.ctypes.data for x in hp] or [None, None]),
                   f.ctypes.data, d_out, n_ciphertexts, kbits, mode, stream)

    def pow_records(self, d_base, d_exp, d_out, n_ciphertexts, stream=0):
        self._call(self.L.cofhe_hip_pow_records, d_base, d_exp, d_out, n_ciphertexts, stream)

    def scal_matmul_records(self, d_cts, d_exp, d_zero, d_out, n, m, p, stream=0):
        self._call(self.L.cofhe_hip_scal_matmul_records, d_cts, d_exp, d_zero, d_out, n, m, p, stream)

    def matmul_plain_ct_records(self, d_s, d_cts, d_zero, d_out, n, m, p, stream=0):
        """out[i,k] = zero o prod_j cts[j,k]^s[i,j]: s n x m exponent records, cts m x p, out n x p; scal_matmul_records on
        transposed views (temporaries from the block cache); d_out must not overlap an input"""
        self._call(self.L.cofhe_hip_matmul_plain_ct_records, d_s, d_cts, d_zero, d_out, n, m, p, stream)

    def conv2d_plain_ct_records(self, d_w, d_cts, d_zero, d_out, image, filters, stride=(1, 1), pad=(0, 0), stream=0, dilation=(1, 1), groups=1):
        """out [B, Ho, Wo, Co] = the convolution of the ciphertext image d_cts [B, H, W, C] = `image` with the plaintext filters
        d_w [kh, kw, C / groups, Co] = `filters` (exponent records), channels last, from the ciphertext d_zero; d_out must not
        overlap an input.  Returns (Ho, Wo)"""
        if tuple(dilation) == (1, 1) and groups == 1:
            shp = _conv_shape(image, filters, stride, pad)
            self._call(self.L.cofhe_hip_conv2d_plain_ct_records, d_w, d_cts, d_zero, d_out, C.byref(shp), stream)
        else:
            geo = _conv_geometry(image, filters, stride, pad, dilation, groups)
            self._call(self.L.cofhe_hip_conv2d_grouped_plain_ct_records, d_w, d_cts, d_zero, d_out, C.byref(geo), stream)
        return conv2d_out_shape(image, filters, stride, pad, dilation, groups)

    def conv2d_out_shape(self, image, filters, stride=(1, 1), pad=(0, 0), dilation=(1, 1), groups=1):
        """(Ho, Wo) of the convolution, or CofheHipError for a geometry it refuses (host only: the module's conv2d_out_shape)"""
        return conv2d_out_shape(image, filters, stride, pad, dilation, groups)

    def sum_pool2d_records(self, d_cts, d_zero, d_out, image, kernel, stride=None, pad=(0, 0), stream=0):
        """out [B, Ho, Wo, C] = the sums over kernel = (kh, kw) windows of the ciphertext image d_cts [B, H, W, C] = `image`,
        channel by channel, from the ciphertext d_zero; stride defaults to the kernel.  Returns (Ho, Wo)"""
        stride = kernel if stride is None else stride
        B, H, W, Cin = image
        geo = _ConvGeometry(B, H, W, Cin, kernel[0], kernel[1], Cin, stride[0], stride[1], pad[0], pad[1], 1, 1, max(Cin, 1))
        self._call(self.L.cofhe_hip_sum_pool2d_records, d_cts, d_zero, d_out, C.byref(geo), stream)
        ho, wo = C.c_uint32(), C.c_uint32()
        _chk(self.L.cofhe_hip_conv2d_geometry_out_shape(C.byref(geo), C.byref(ho), C.byref(wo)))
        return int(ho.value), int(wo.value)

    def matmul_plain_plain_records(self, d_a, d_b, d_out, n, m, p, kbits, stream=0):
        """out = a (n x m) . b (m x p) mod 2^kbits on exponent records, outputs in [0, 2^k) with sign word 0; one launch,
        purely stream-ordered"""
        self._call(self.L.cofhe_hip_matmul_plain_plain_records, d_a, d_b, d_out, n, m, p, kbits, stream)

    def conv2d_plain_plain_records(self, d_img, d_w, d_out, image, filters, kbits, stride=(1, 1), pad=(0, 0), stream=0, dilation=(1, 1)):
        """out [B, Ho, Wo, Co] = the convolution mod 2^kbits of the plaintext image d_img [B, H, W, C] = `image` with the plaintext
        filters d_w [kh, kw, C, Co] = `filters`, all exponent records, channels last; outputs in [0, 2^k) with sign word 0; one
        launch, purely stream-ordered.  The E * D term of a convolution Beaver triplet.  Returns (Ho, Wo)"""
        geo = _conv_geometry(image, filters, stride, pad, dilation, 1)
        self._call(self.L.cofhe_hip_conv2d_plain_plain_records, d_img, d_w, d_out, C.byref(geo), kbits, stream)
        return conv2d_out_shape(image, filters, stride, pad, dilation, 1)

    def conv2d_ct_filters_records(self, d_img_exps, d_filters_cts, d_zero, d_out, image, filters, stride=(1, 1), pad=(0, 0), stream=0,
                                  dilation=(1, 1)):
        """out [B, Ho, Wo, Co] = the convolution of the PLAINTEXT image d_img_exps [B, H, W, C] = `image` (exponent records) with the
        CIPHERTEXT filters d_filters_cts [kh, kw, C, Co] = `filters`, channels last, from the ciphertext d_zero; d_out must not
        overlap an input.  The E * [Bf] term of a convolution Beaver triplet.  Returns (Ho, Wo)"""
        geo = _conv_geometry(image, filters, stride, pad, dilation, 1)
        self._call(self.L.cofhe_hip_conv2d_ct_filters_records, d_img_exps, d_filters_cts, d_zero, d_out, C.byref(geo), stream)
        return conv2d_out_shape(image, filters, stride, pad, dilation, 1)

    def pow_dot_records(self, d_bases, d_exps, d_out, n_ciphertexts, d, stream=0):
        """out[e] = prod_{i<d} bases[i][e]^exps[i][e]: d ciphertext tensors and d exponent tensors of n elements, power-major,
        one ladder per record with shared squarings (1 <= d <= 8); d_out must not overlap an input"""
        self._call(self.L.cofhe_hip_pow_dot_records, d_bases, d_exps, d_out, n_ciphertexts, d, stream)

    def poly_shift_records(self, d_coef, d_x, d_q, n, d, kbits, stream=0):
        """q[i n + e] = sum_{j>=i} C(j,i) coef[j] x[e]^(j-i) mod 2^kbits, i <= d, on exponent records (coef: d + 1, x: n,
        q: (d + 1) n, power-major); outputs in [0, 2^k) with sign word 0"""
        self._call(self.L.cofhe_hip_poly_shift_records, d_coef, d_x, d_q, n, d, kbits, stream)

    def poly_close_records(self, d_coef, d_e, d_powers, f_record, d_out, n_ciphertexts, d, kbits, stream=0):
        """the closing step of a polynomial evaluation: out[e] = (prod_{i=1..d} powers[i-1][e]^q_i(e[e])) o f^q_0(e[e]) with q the
        Taylor shift of coef (d + 1 exponent records) at the opened values e (n exponent records); powers: d tensors [a^i],
        power-major; f_record: host uint32[168]; d_out must not overlap an input"""
        f = _host_record(f_record)
        self._call(self.L.cofhe_hip_poly_close_records, d_coef, d_e, d_powers, f.ctypes.data, d_out, n_ciphertexts, d, kbits, stream)

    def divfloor_plain_records(self, d_v, d_div, n_div, d_q, n, kbits, stream=0):
        """q[e] = floor(s(v[e]) / div[e mod n_div]) mod 2^kbits on exponent records, s the centred residue (v: n, div: n_div,
        q: n); 1 <= div < 2^(kbits-1), else quotient 0 and bit 4 of device_status; outputs in [0, 2^k) with sign word 0"""
        self._call(self.L.cofhe_hip_divfloor_plain_records, d_v, d_div, n_div, d_q, n, kbits, stream)

    def div_close_records(self, d_e, d_div, n_div, d_rq, f_record, d_out, n_ciphertexts, kbits, stream=0):
        """the closing step of a division by public divisors: out[e] = (c1, c2 o f^e_q) of rq[e] with e_q = floor(s(e[e]) /
        div[e mod n_div]) mod 2^kbits; e: n exponent records of the opened values x - r, rq: the [r_q] of the division pairs;
        f_record: host uint32[168]; d_out must not overlap an input"""
        f = _host_record(f_record)
        self._call(self.L.cofhe_hip_div_close_records, d_e, d_div, n_div, d_rq, f.ctypes.data, d_out, n_ciphertexts, kbits, stream)

    def divmod_plain_records(self, d_v, d_div, n_div, d_q, d_rem, n, rows, kbits, stream=0):
        """q[e] = floor(s(v[e]) / D) mod 2^kbits on exponent records and rem[e] = s(v[e]) - D q(v[e]) in [0, D) as uint32, D =
        div[e mod n_div]; 1 <= D <= rows <= 4096 and D < 2^(kbits-1), else quotient 0, remainder 0 and bit 4 of device_status"""
        self._call(self.L.cofhe_hip_divmod_plain_records, d_v, d_div, n_div, d_q, d_rem, n, rows, kbits, stream)

    def divx_rows_records(self, d_r, d_div, n_div, d_out, n, rows, kbits, stream=0):
        """out[i rows + j] = (q(r[i]) + [m(r[i]) + j >= D]) mod 2^kbits for j < D = div[i mod n_div] and the zero record for D <= j <
        rows, on exponent records (r: n, div: n_div, out: n rows): the plaintext rows of the exact-division tuples; d_out must not
        overlap an input"""
        self._call(self.L.cofhe_hip_divx_rows_records, d_r, d_div, n_div, d_out, n, rows, kbits, stream)

    def divx_tuples_records(self, d_r, d_div, n_div, d_rho, h_record, pk_record, f_record, d_out, n, rows, kbits, stream=0):
        """the entries of n exact-division tuples: divx_rows_records, then encrypt_fresh_records over the n rows plaintexts with the
        randomness rho (n rows exponent records, each used once); h_record, pk_record, f_record: host uint32[168]; d_out: n rows
        ciphertexts"""
        h, pk, f = _host_record(h_record), _host_record(pk_record), _host_record(f_record)
        self._call(self.L.cofhe_hip_divx_tuples_records, d_r, d_div, n_div, d_rho, h.ctypes.data, pk.ctypes.data, f.ctypes.data, d_out, n,
                   rows, kbits, stream)

    def divx_close_records(self, d_e, d_div, n_div, d_tuples, rows, f_record, d_out, n, kbits, stream=0):
        """the closing step of an exact division: out[i] = (c1, c2 o f^q(e[i])) of tuples[i rows + m(e[i])]; e: n exponent records
        of the opened values x - r, tuples: n rows ciphertexts; f_record: host uint32[168]; d_out must not overlap an input"""
        f = _host_record(f_record)
        self._call(self.L.cofhe_hip_divx_close_records, d_e, d_div, n_div, d_tuples, rows, f.ctypes.data, d_out, n, kbits, stream)

    def divx_shape(self, shape_e, shape_t) -> int:
        """host only: rows of the tuples (shape_t = shape_e + [rows]) that go with opened values of shape_e; COFHE_HIP_ESHAPE otherwise"""
        rows = C.c_uint32()
        _chk(self.L.cofhe_hip_divx_shape(len(shape_e), _u32s(shape_e), len(shape_t), _u32s(shape_t), C.byref(rows)))
        return rows.value

    def lut_rotate_records(self, d_table, n_tab, d_r, d_out, n, bits, stream=0):
        """out[i 2^bits + j] = table[(i mod n_tab) 2^bits + ((j + r[i]) mod 2^bits)] on exponent records (table: n_tab 2^bits, r: n,
        out: n 2^bits): the plaintext rows of the lookup tuples; 1 <= bits <= 12; d_out must not overlap an input"""
        self._call(self.L.cofhe_hip_lut_rotate_records, d_table, n_tab, d_r, d_out, n, bits, stream)

    def lut_tuples_records(self, d_table, n_tab, d_r, d_rho, h_record, pk_record, f_record, d_out, n, bits, kbits, stream=0):
        """the entries of n lookup tuples: lut_rotate_records, then encrypt_fresh_records over the n 2^bits rows with the randomness
        rho (n 2^bits exponent records, each used once); h_record, pk_record, f_record: host uint32[168]; d_out: n 2^bits
        ciphertexts"""
        h, pk, f = _host_record(h_record), _host_record(pk_record), _host_record(f_record)
        self._call(self.L.cofhe_hip_lut_tuples_records, d_table, n_tab, d_r, d_rho, h.ctypes.data, pk.ctypes.data, f.ctypes.data, d_out, n,
                   bits, kbits, stream)

    def lut_tuples_shape_bits(self, shape_e, shape_t) -> int:
        """host only: bits of the tuples (shape_t = shape_e + [2^bits]) that go with opened values of shape_e; COFHE_HIP_ESHAPE otherwise"""
        bits = C.c_uint32()
        _chk(self.L.cofhe_hip_lut_tuples_shape_bits(len(shape_e), _u32s(shape_e), len(shape_t), _u32s(shape_t), C.byref(bits)))
        return bits.value

    def lut_select_records(self, d_e, d_tuples, d_out, n, bits, stream=0):
        """the closing step of a lookup: out[i] = tuples[i 2^bits + (e[i] mod 2^bits)], ciphertexts copied byte for byte; e: n
        exponent records of the opened values x - r; d_out must not overlap an input"""
        self._call(self.L.cofhe_hip_lut_select_records, d_e, d_tuples, d_out, n, bits, stream)

    def view_records(self, view, d_src, d_fill, d_dst, words, stream=0):
        """the box of an affine view (a View; module functions view_permute and kin build them) of records of `words` dwords:
        dst[view_dest(i)] = src[view_source(i)], or the one record at d_fill (0: none, for a view that needs no fill) where the view
        reads outside its source; the rest of the destination is not written.  A byte-for-byte copy: nothing is re-randomised."""
        self._call(self.L.cofhe_hip_view_records, C.byref(view), d_src, d_fill, d_dst, words, stream)

    def gather_records(self, d_src, n_src, d_index, d_fill, d_dst, n_out, words, stream=0):
        """dst[i] = src[index[i]] for the n_out uint32 at d_index: GATHER_FILL writes the record at d_fill, GATHER_KEEP leaves dst[i]
        alone, another index >= n_src writes the fill record (with d_fill 0: leaves dst[i] alone) and sets bit 32 of the status word"""
        self._call(self.L.cofhe_hip_gather_records, d_src, n_src, d_index, d_fill, d_dst, n_out, words, stream)

    def view_tensor_bytes(self, data: bytes, view, fill: bytes = None, kind: int = 2) -> bytes:
        """a serialised tensor (kind 2 ciphertexts / 1 partial decryptions / 0 plaintexts) whose shape is the view's source ->
        the serialised tensor of the view's destination shape; `fill`: a serialised one-element tensor of the same kind, for a
        view that reads outside its source.  Composed here from unpack_tensor_device (which validates the incoming forms),
        view_records and pack_tensor_device: the library has no entry point of its own for it.  The destination outside the
        view's box is not written, so a view placed in a larger destination (view_into) is refused."""
        per = {2: 2, 1: 1, 0: 1}[kind]                               # records per element
        rec_words = REC_WORDS if kind else EXP_REC_WORDS
        n_src, n_box, n_dst, needs_fill = view_check(view)
        if n_box != n_dst:
            raise CofheHipError(COFHE_HIP_EINVAL, "view_tensor_bytes: the view's box is not its whole destination")
        with _DeviceScope(self) as dev:
            dsrc, shape, n = dev.load(data, kind)
            if list(shape) != [int(view.src_extent[a]) for a in range(view.src_ndim)] or n != per * n_src:
                raise CofheHipError(COFHE_HIP_ESHAPE, "view_tensor_bytes: the tensor's shape is not the view's source")
            dfill = 0
            if fill is not None:
                dfill, _, nf = dev.load(fill, kind)
                if nf != per:
                    raise CofheHipError(COFHE_HIP_ESHAPE, "view_tensor_bytes: the fill is a tensor of one element")
            out_shape = [int(view.dst_extent[d]) for d in range(view.out_ndim)]
            dout = dev.alloc(max(n_dst, 1) * per * rec_words * 4)
            self.view_records(view, dsrc, dfill, dout, per * rec_words)
            return dev.packed(dout, per * n_dst, kind, out_shape)

    def spline_rows_records(self, d_pieces, n_tab, d_r, d_out, n, bits, shift, d, kbits, stream=0):
        """the plaintext rows of n spline tuples on exponent records: out[(i 2^bits + j) (d + 1) + c] = coefficient c of the Taylor
        shift of piece (j + rho_i) mod 2^bits of table i mod n_tab at r_i minus the piece's origin, rho_i = bits shift .. shift + bits
        - 1 of r_i mod 2^kbits (pieces: n_tab 2^bits (d + 1), r: n, out: n 2^bits (d + 1)); d_out must not overlap an input"""
        self._call(self.L.cofhe_hip_spline_rows_records, d_pieces, n_tab, d_r, d_out, n, bits, shift, d, kbits, stream)

    def spline_tuples_records(self, d_pieces, n_tab, d_r, d_rho, h_record, pk_record, f_record, d_out, n, bits, shift, d, kbits, stream=0):
        """the entries of n spline tuples: spline_rows_records, then encrypt_fresh_records over the n 2^bits (d + 1) rows with the
        randomness rho (as many exponent records, each used once); h_record, pk_record, f_record: host uint32[168]; d_out:
        n 2^bits (d + 1) ciphertexts"""
        h, pk, f = _host_record(h_record), _host_record(pk_record), _host_record(f_record)
        self._call(self.L.cofhe_hip_spline_tuples_records, d_pieces, n_tab, d_r, d_rho, h.ctypes.data, pk.ctypes.data, f.ctypes.data, d_out,
                   n, bits, shift, d, kbits, stream)

    def spline_tuples_shape(self, shape_e, shape_t):
        """host only: (bits, d) of the tuples (shape_t = shape_e + [2^bits, d + 1]) that go with opened values of shape_e;
        COFHE_HIP_ESHAPE otherwise"""
        bits, d = C.c_uint32(), C.c_uint32()
        _chk(self.L.cofhe_hip_spline_tuples_shape(len(shape_e), _u32s(shape_e), len(shape_t), _u32s(shape_t), C.byref(bits), C.byref(d)))
        return bits.value, d.value

    def spline_powers_records(self, d_e, d_out, n, d, kbits, stream=0):
        """out[(c - 1) n + i] = e[i]^c mod 2^kbits, c = 1 .. d, on exponent records (e: n, out: d n, power-major)"""
        self._call(self.L.cofhe_hip_spline_powers_records, d_e, d_out, n, d, kbits, stream)

    def spline_close_records(self, d_e, d_tuples, d_out, n, bits, shift, d, kbits, stream=0):
        """the closing step of a spline: out[i] = [q_{j,0}] o prod_{c=1..d} [q_{j,c}]^(e[i]^c mod 2^kbits) over row j = bits shift ..
        shift + bits - 1 of e[i] of element i's tuple; e: n exponent records of the opened values x - r, tuples: n 2^bits (d + 1)
        ciphertexts; d_out must not overlap an input"""
        self._call(self.L.cofhe_hip_spline_close_records, d_e, d_tuples, d_out, n, bits, shift, d, kbits, stream)

    def cmp_rows_records(self, d_r, d_out, n, bits, digit_bits, kbits, stream=0):
        """the plaintext rows of n comparison tuples on exponent records: out[(i nd + j) 2^d + c] = 2^j sgn(r_ij - c), r_ij digit j
        of r[i] mod 2^bits, nd = ceil(bits / d) (r: n, out: n nd 2^d); d_out must not overlap d_r"""
        self._call(self.L.cofhe_hip_cmp_rows_records, d_r, d_out, n, bits, digit_bits, kbits, stream)

    def cmp_tuples_records(self, d_r, d_rho, h_record, pk_record, f_record, d_out, n, bits, digit_bits, kbits, stream=0):
        """the entries of n comparison tuples: cmp_rows_records, then encrypt_fresh_records over the n nd 2^d rows with the
        randomness rho (as many exponent records, each used once); h_record, pk_record, f_record: host uint32[168]; d_out:
        n nd 2^d ciphertexts"""
        h, pk, f = _host_record(h_record), _host_record(pk_record), _host_record(f_record)
        self._call(self.L.cofhe_hip_cmp_tuples_records, d_r, d_rho, h.ctypes.data, pk.ctypes.data, f.ctypes.data, d_out, n, bits, digit_bits,
                   kbits, stream)

    def cmp_shape(self, bits, digit_bits, kbits, shape_e=None, shape_t=None):
        """host only: (nd, nd 2^d) of a comparison on a window of `bits` bits in digits of digit_bits bits (COFHE_HIP_EINVAL for
        the parameter bounds); with shape_t, also COFHE_HIP_ESHAPE unless shape_t = shape_e + [nd, 2^d]"""
        nd, entries = C.c_uint32(), C.c_uint32()
        se, st = list(shape_e or []), shape_t
        _chk(self.L.cofhe_hip_cmp_shape(bits, digit_bits, kbits, len(se), _u32s(se), len(st) if st is not None else 0,
                                        _u32s(st) if st is not None else None, C.byref(nd), C.byref(entries)))
        return nd.value, entries.value

    def cmp_close_records(self, d_e, d_tuples, d_out, d_wrap, n, bits, digit_bits, kbits, stream=0):
        """the closing step of a comparison's first round: out[2 i + s] = the product of the nd entries of element i's tuple that
        threshold s (A, then B) of e[i] mod 2^bits selects, wrap[i] = [A > B]; e: n exponent records of the opened values x - r,
        tuples: n nd 2^d ciphertexts, out: 2 n ciphertexts, wrap: n exponent records; the outputs must not overlap an input"""
        self._call(self.L.cofhe_hip_cmp_close_records, d_e, d_tuples, d_out, d_wrap, n, bits, digit_bits, kbits, stream)

    def decrypt_records(self, d_cts, d_sk, f_record, d_out, n_ciphertexts, kbits, stream=0):
        """f_record: host numpy uint32[168]; d_out: n * (ceil(k/32) + 1) words"""
        f = _host_record(f_record)
        self._call(self.L.cofhe_hip_decrypt_records, d_cts, d_sk, f.ctypes.data, d_out, n_ciphertexts, kbits, stream)

    def accumulate_records(self, d_x, d_zero, d_out, n, m, p, stream=0):
        """out[i,k] = zero o prod_j x[i,j,k] (x: n*m*p ciphertexts, out: n*p)"""
        self._call(self.L.cofhe_hip_accumulate_records, d_x, d_zero, d_out, n, m, p, stream)

    def pow_form_records(self, d_base, d_exp, d_out, n_forms, stream=0):
        self._call(self.L.cofhe_hip_pow_form_records, d_base, d_exp, d_out, n_forms, stream)

    def pow_fixed_base_record(self, base_record, exp_record, d_out, stream=0):
        """base_record (168 u32) and exp_record (32 u32) are host numpy arrays; d_out one device record.  The
        context caches the table base^(2^j) of the last few bases."""
        b, e = _host_record(base_record), _host_record(exp_record, EXP_REC_WORDS)
        self._call(self.L.cofhe_hip_pow_fixed_base_record, b.ctypes.data, e.ctypes.data, d_out, stream)

    def pow_fixed_base_records(self, base_records, exp_records, d_out, stream=0):
        """n <= 4 fixed-base powers in one product tree; base_records n x 168 u32, exp_records n x 32 u32 (host)"""
        import numpy as np
        b = np.ascontiguousarray(base_records, dtype=np.uint32).reshape(-1)
        e = np.ascontiguousarray(exp_records, dtype=np.uint32).reshape(-1)
        n = b.size // REC_WORDS
        assert b.size == n * REC_WORDS and e.size == n * EXP_REC_WORDS
        self._call(self.L.cofhe_hip_pow_fixed_base_records, n, b.ctypes.data, e.ctypes.data, d_out, stream)

    def encrypt_records(self, d_plain, d_c1_pkr, f_record, d_out, n_ciphertexts, kbits, stream=0):
        """d_plain: n exponent records; d_c1_pkr: records of h^r and pk^r; d_out: 2n records"""
        f = _host_record(f_record)
        self._call(self.L.cofhe_hip_encrypt_records, d_plain, d_c1_pkr, f.ctypes.data, d_out, n_ciphertexts, kbits, stream)

    def pow_fixed_base_many_records(self, base_record, d_exps, d_out, n, stream=0):
        """out[i] = base^e[i] by the fixed-base comb: base_record a host uint32[168], d_exps n exponent records, d_out n records"""
        b = _host_record(base_record)
        self._call(self.L.cofhe_hip_pow_fixed_base_many_records, b.ctypes.data, d_exps, d_out, n, stream)

    def encrypt_fresh_records(self, d_plain, d_r, h_record, pk_record, f_record, d_out, n_ciphertexts, kbits, stream=0):
        """out[i] = (h^r_i, pk^r_i o f^(m_i mod 2^k)): one r per ciphertext (d_r: n exponent records); h, pk, f host records"""
        h, pk, f = _host_record(h_record), _host_record(pk_record), _host_record(f_record)
        self._call(self.L.cofhe_hip_encrypt_fresh_records, d_plain, d_r, h.ctypes.data, pk.ctypes.data, f.ctypes.data, d_out, n_ciphertexts,
                   kbits, stream)

    def rerandomize_records(self, d_cts, d_r, h_record, pk_record, d_out, n_ciphertexts, stream=0):
        """out[i] = (c1_i o h^r_i, c2_i o pk^r_i); d_out may be d_cts"""
        h, pk = _host_record(h_record), _host_record(pk_record)
        self._call(self.L.cofhe_hip_rerandomize_records, d_cts, d_r, h.ctypes.data, pk.ctypes.data, d_out, n_ciphertexts, stream)

    def part_decrypt_records(self, d_cts, d_share, d_out, n_ciphertexts, stream=0):
        """d_out: n form records = c1^share"""
        self._call(self.L.cofhe_hip_part_decrypt_records, d_cts, d_share, d_out, n_ciphertexts, stream)

    def combine_part_decryptions_records(self, d_cts, d_parts, lambdas, f_record, d_out, n_ciphertexts, kbits, stream=0):
        """d_parts: len(lambdas) x n form records (party-major); lambdas: +1 / -1 per party"""
        f = _host_record(f_record)
        lam = (C.c_int32 * len(lambdas))(*lambdas)
        self._call(self.L.cofhe_hip_combine_part_decryptions_records, d_cts, d_parts, len(lambdas), lam, f.ctypes.data, d_out,
                   n_ciphertexts, kbits, stream)

    # ---- device memory and fences of the library's own HIP runtime (bench.py uses no other) --------------------
    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._call(self.L.cofhe_hip_malloc, nbytes, C.byref(p))
        return p.value

    def free(self, dptr: int, stream=0):
        self._call(self.L.cofhe_hip_free_on_stream, dptr, stream)

    def upload(self, dptr: int, host, stream=0):
        """host: a contiguous numpy array (or bytes); copies all of it to dptr"""
        import numpy as np
        a = np.frombuffer(host, dtype=np.uint8) if isinstance(host, (bytes, bytearray)) else np.ascontiguousarray(host)
        self._call(self.L.cofhe_hip_upload, dptr, a.ctypes.data, a.nbytes, stream)
        self._call(self.L.cofhe_hip_stream_sync, stream)       # the host array may go away after the call

    def download(self, dptr: int, nbytes: int, dtype="uint32", stream=0):
        """device -> a new numpy array of `dtype` (synchronises the stream)"""
        import numpy as np
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        self._call(self.L.cofhe_hip_download, out.ctypes.data, dptr, out.nbytes, stream)
        return out

    def stream_sync(self, stream=0):
        self._call(self.L.cofhe_hip_stream_sync, stream)

    def stream_create(self, nonblocking=1) -> int:
        """a stream of the library's own HIP runtime on the context's device (a torch.cuda.Stream handle belongs to torch's
        runtime and means nothing to the library); nonblocking: the null stream does not order it"""
        s = C.c_void_p()
        self._call(self.L.cofhe_hip_stream_create, 1 if nonblocking else 0, C.byref(s))
        return s.value

    def stream_destroy(self, stream):
        """waits for the work queued on the stream, then releases it; 0 / None is a no-op"""
        self._call(self.L.cofhe_hip_stream_destroy, stream)

    def stream_query(self, stream=0) -> int:
        """1 while work queued on the stream is pending, 0 when it is idle; does not wait"""
        busy = C.c_int()
        self._call(self.L.cofhe_hip_stream_query, stream, C.byref(busy))
        return int(busy.value)

    def profile_read(self, kernel: str, clear=False):
        """(summed ms, launches) of the spans the "profile_kernels" option recorded for `kernel`"""
        ms, n = C.c_float(), C.c_uint32()
        self._call(self.L.cofhe_hip_profile_read, kernel.encode(), C.byref(ms), C.byref(n), 1 if clear else 0)
        return float(ms.value), int(n.value)

    # ---- more than one GPU (cofhe_amd/csrc/shard.hip) -------------------------------------------------------
    def shard_rows(self, n_rows, world, rank):
        """(row0, n_local) of this rank's contiguous row block"""
        r0, nl = C.c_uint64(), C.c_uint64()
        self.L.cofhe_hip_shard_rows(n_rows, world, rank, C.byref(r0), C.byref(nl))
        return r0.value, nl.value

    def comm_unique_id(self) -> bytes:
        buf = (C.c_uint8 * 128)()
        _chk(self.L.cofhe_hip_comm_unique_id(buf))
        return bytes(buf)

    def comm_create(self, unique_id: bytes, world: int, rank: int):
        comm = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._call(self.L.cofhe_hip_comm_create, buf, world, rank, C.byref(comm))
        return comm

    def comm_info(self, comm):
        """(world, rank, rank count RCCL reports for the communicator)"""
        w, r, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _chk(self.L.cofhe_hip_comm_info(comm, C.byref(w), C.byref(r), C.byref(n)))
        return w.value, r.value, n.value

    def comm_set_option(self, comm, name: str, value: int):
        _chk(self.L.cofhe_hip_comm_set_option(comm, name.encode(), value))

    def comm_destroy(self, comm):
        self.L.cofhe_hip_comm_destroy(comm)

    def all_gather_rows(self, comm, d_local, n_rows, row_bytes, d_out, stream=0):
        self._call(self.L.cofhe_hip_all_gather_rows, comm, d_local, n_rows, row_bytes, d_out, stream)

    def set_option(self, name: str, value: int):
        """pins a launcher decision of the matrix product ("wnaf_width", "matmul_segments"; 0 = automatic)"""
        self._call(self.L.cofhe_hip_ctx_set_option, name.encode(), value)

    def device_status(self, clear=True, stream=0) -> int:
        """status word of the kernels (bit 1: Euclid cap, 2: reduction cap, 4: division; 32: gather_records met an index beyond
        its source and wrote the fill record): 0 unless a record was not a form or an index was bad"""
        w = C.c_uint32()
        self._call(self.L.cofhe_hip_device_status, C.byref(w), 1 if clear else 0, stream)
        return w.value

    def validate_records(self, d_records, n_records, stream=0) -> bool:
        """True when every record is a reduced form of the context's discriminant"""
        ok = C.c_int()
        self._call(self.L.cofhe_hip_validate_records, d_records, n_records, C.byref(ok), stream)
        return bool(ok.value)

    def time_compose(self, d_a, d_b, d_out, n_records, iters, stream=0) -> float:
        ms = C.c_float()
        self._call(self.L.cofhe_hip_time_compose, d_a, d_b, d_out, n_records, iters, stream, C.byref(ms))
        return float(ms.value)

    def time_stream(self, fn, iters=1, stream=0) -> float:
        """milliseconds per call of `iters` calls of fn() between two HIP events on `stream` (cofhe_hip_timer_*): the
        stream the library launches on"""
        h = C.c_void_p()
        self._call(self.L.cofhe_hip_timer_start, stream, C.byref(h))
        try:
            for _ in range(iters):
                fn()
        finally:
            ms = C.c_float()
            rc = self.L.cofhe_hip_timer_stop(self.ctx, h, stream, C.byref(ms))
        _chk(rc)
        return float(ms.value) / iters


def workspace_plan(op: str, *args):
    """cofhe_hip_workspace_plan (host only): ([(name, byte offset, byte count)], total bytes) -- how the entry point `op`
    carves the context's workspace for these operand counts (the launchers use the same plan functions)"""
    L = load_library()

    class Region(C.Structure):
        _fields_ = [("name", C.c_char * 24), ("offset", C.c_uint64), ("bytes", C.c_uint64)]

    regs = (Region * 8)()
    n, total = C.c_uint32(), C.c_uint64()
    _chk(L.cofhe_hip_workspace_plan(op.encode(), _u64s(args), len(args), regs, 8, C.byref(n), C.byref(total)))
    return [(regs[i].name.decode(), int(regs[i].offset), int(regs[i].bytes)) for i in range(n.value)], int(total.value)


class _ConvShape(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("B", "H", "W", "C", "kh", "kw", "Co", "sh", "sw", "ph", "pw")]


def _conv_shape(image, filters, stride, pad):
    B, H, W, Cin = image
    kh, kw, Cf, Co = filters
    if Cf != Cin:
        raise CofheHipError(COFHE_HIP_ESHAPE, "conv2d: the channels of the filters and of the image differ")
    return _ConvShape(B, H, W, Cin, kh, kw, Co, stride[0], stride[1], pad[0], pad[1])


class _ConvGeometry(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("B", "H", "W", "C", "kh", "kw", "Co", "sh", "sw", "ph", "pw", "dh", "dw", "groups")]


def _conv_geometry(image, filters, stride, pad, dilation, groups):
    B, H, W, Cin = image
    kh, kw, Cf, Co = filters
    if groups > 0 and Cf != Cin // groups:
        raise CofheHipError(COFHE_HIP_ESHAPE, "conv2d: the channels of the filters and of the image differ")
    return _ConvGeometry(B, H, W, Cin, kh, kw, Co, stride[0], stride[1], pad[0], pad[1], dilation[0], dilation[1], groups)


def conv2d_out_shape(image, filters, stride=(1, 1), pad=(0, 0), dilation=(1, 1), groups=1):
    """cofhe_hip_conv2d_out_shape / cofhe_hip_conv2d_geometry_out_shape (host only): (Ho, Wo) of image [B, H, W, C] under filters
    [kh, kw, C / groups, Co]; raises CofheHipError (COFHE_HIP_EINVAL) for a geometry the convolution refuses"""
    L = load_library()
    ho, wo = C.c_uint32(), C.c_uint32()
    if tuple(dilation) == (1, 1) and groups == 1:
        shp = _conv_shape(image, filters, stride, pad)
        _chk(L.cofhe_hip_conv2d_out_shape(C.byref(shp), C.byref(ho), C.byref(wo)))
    else:
        geo = _conv_geometry(image, filters, stride, pad, dilation, groups)
        _chk(L.cofhe_hip_conv2d_geometry_out_shape(C.byref(geo), C.byref(ho), C.byref(wo)))
    return int(ho.value), int(wo.value)


VIEW_MAX_DIMS = 8
GATHER_FILL, GATHER_KEEP = 0xFFFFFFFF, 0xFFFFFFFE


class View(C.Structure):
    """cofhe_hip_view: the box out_extent of a dense row-major source src_extent, source coordinate c_a = start[a] + sum_d
    map[a][d] o_d, placed at dst_start inside a dense row-major destination dst_extent (include/cofhe_hip.h)"""
    _fields_ = [("out_ndim", C.c_uint32), ("src_ndim", C.c_uint32), ("out_extent", C.c_uint64 * 8), ("src_extent", C.c_uint64 * 8),
                ("start", C.c_int64 * 8), ("map", (C.c_int32 * 8) * 8), ("dst_extent", C.c_uint64 * 8), ("dst_start", C.c_uint64 * 8)]

    @property
    def out_shape(self):
        return [int(self.out_extent[d]) for d in range(self.out_ndim)]

    @property
    def dst_shape(self):
        return [int(self.dst_extent[d]) for d in range(self.out_ndim)]


def _u64s(values):
    return (C.c_uint64 * max(1, len(values)))(*[int(x) for x in values])


def _i64s(values):
    return (C.c_int64 * max(1, len(values)))(*[int(x) for x in values])


def view_check(view):
    """cofhe_hip_view_check (host only): (n_src, n_box, n_dst, needs_fill); raises CofheHipError (COFHE_HIP_EINVAL) for more than 8
    axes, a box outside its destination or a source coordinate that can leave 64 bits"""
    ns, nb, nd, nf = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    _chk(load_library().cofhe_hip_view_check(C.byref(view), C.byref(ns), C.byref(nb), C.byref(nd), C.byref(nf)))
    return int(ns.value), int(nb.value), int(nd.value), bool(nf.value)


def view_permute(shape, perm):
    """output axis d is source axis perm[d] (numpy.transpose)"""
    v = View()
    _chk(load_library().cofhe_hip_view_permute(_u64s(shape), len(shape), _u32s(perm), C.byref(v)))
    return v


def view_slice(shape, start, stop, step):
    """src[start:stop:step] per axis, bounds in range; with a negative step a stop of -1 means down to and including element 0"""
    v = View()
    _chk(load_library().cofhe_hip_view_slice(_u64s(shape), len(shape), _i64s(start), _i64s(stop), _i64s(step), C.byref(v)))
    return v


def view_pad(shape, lo, hi):
    v = View()
    _chk(load_library().cofhe_hip_view_pad(_u64s(shape), len(shape), _u64s(lo), _u64s(hi), C.byref(v)))
    return v


def view_broadcast(shape, out_shape):
    """numpy's rule, right-aligned"""
    v = View()
    _chk(load_library().cofhe_hip_view_broadcast(_u64s(shape), len(shape), _u64s(out_shape), len(out_shape), C.byref(v)))
    return v


def view_window_taps(image, kernel, stride=(1, 1), pad=(0, 0), dilation=(1, 1)):
    """[B, H, W, C] -> [kh, kw, B, Ho, Wo, C]: tap (dy, dx) of every window, the fill record in the padding"""
    B, H, W, Cin = image
    geo = _ConvGeometry(B, H, W, Cin, kernel[0], kernel[1], Cin, stride[0], stride[1], pad[0], pad[1], dilation[0], dilation[1], 1)
    v = View()
    _chk(load_library().cofhe_hip_view_window_taps(C.byref(geo), C.byref(v)))
    return v


def view_into(view, dst_shape, dst_start):
    """the same view with its box at dst_start inside a destination of dst_shape (a new View)"""
    v = View.from_buffer_copy(view)
    _chk(load_library().cofhe_hip_view_into(C.byref(v), _u64s(dst_shape), _u64s(dst_start)))
    return v


COMB_POWERS, COMB_ENCRYPT, COMB_RERANDOMIZE = 0, 1, 2


def comb_shape(kind: int, n: int, exp_bits: int, kbits: int = 0, w: int = 0, chunk: int = 0):
    """cofhe_hip_comb_shape (host only): (w, slots per output record, items per pass) the comb launcher takes for n items of
    `kind` whose longest exponent has exp_bits bits; w / chunk pin the "comb_width" / "comb_chunk" options (0: automatic)"""
    ow, sl, ch = C.c_uint32(), C.c_uint32(), C.c_uint64()
    _chk(load_library().cofhe_hip_comb_shape(kind, n, exp_bits, kbits, w, chunk, C.byref(ow), C.byref(sl), C.byref(ch)))
    return int(ow.value), int(sl.value), int(ch.value)


def gather_plan(n_rows: int, row_bytes: int, world: int):
    """cofhe_hip_gather_plan (host only): ([(byte offset, byte count)] per rank, uniform) -- the collective the
    library will run for a row-sharded tensor"""
    offs = (C.c_uint64 * world)()
    cnts = (C.c_uint64 * world)()
    uni = C.c_int()
    _chk(load_library().cofhe_hip_gather_plan(n_rows, row_bytes, world, offs, cnts, C.byref(uni)))
    return [(int(offs[r]), int(cnts[r])) for r in range(world)], bool(uni.value)
