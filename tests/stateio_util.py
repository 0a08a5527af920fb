"""What the CPU and GPU tests of the device state I/O share: a numpy restatement of the wave-tile layout off(w, i) (DESIGN.md section
3), independent of ekf_layout.hpp, the record words `qle_set_state` writes restated from include/qle_ekf.h, and the expected result of
a copy.  Every comparison of these tests is bit for bit: the feature moves and rounds words and computes nothing else."""
import numpy as np

SW, XW, PW, PWC = 144, 16, 120, 48
RECORD_WORDS = {False: 136, True: 64}
NP_T = {"f32": np.float32, "f64": np.float64}
# the six record kinds: name -> (dtype, num_states, compact); full9 is what an est_bias = 0 handle holds unless compact records are chosen
KINDS = {"f32-full": ("f32", 15, False), "f32-full9": ("f32", 9, False), "f32-compact": ("f32", 9, True),
         "f64-full": ("f64", 15, False), "f64-full9": ("f64", 9, False), "f64-compact": ("f64", 9, True)}


def padded(B):
    return -(-B // 64) * 64


def off(w, i, dtype, WT=SW):
    """off(w, i) = (i/64)*WT*64 + ((w/VW)*64 + i%64)*VW + w%VW, VW = 4 (fp32) / 2 (fp64): whole quad rows only (WT % VW == 0)."""
    VW = 4 if dtype == "f32" else 2
    w, i = np.asarray(w, np.int64), np.asarray(i, np.int64)
    return (i // 64) * WT * 64 + ((w // VW) * 64 + i % 64) * VW + w % VW


def record_offsets(B, dtype, words, WT=SW):
    """[B, words] array offsets of words 0..words-1 of filters 0..B-1"""
    return off(np.arange(words)[None, :], np.arange(B)[:, None], dtype, WT)


def bits(a):
    """a float array as unsigned integers of its width: NaN payloads and signed zeros compare"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def sidx(i, k):
    """Order of the 120 covariance words of a full record: 5 x 5 blocks of 3 x 3, block-row after block-row;
    quad-lane l holds column l of every block (b, c), c > b, and two entries of each diagonal block; memory quad 3m + l is the m-th
    quad of lane l."""
    i, k = min(i, k), max(i, k)
    base = [0, 14, 25, 33, 38]
    b, c, ii, kk = i // 3, k // 3, i % 3, k % 3
    if b < c:
        lane, pos = kk, base[b] + 2 + 3 * (c - b - 1) + ii
    elif ii == kk:
        lane, pos = kk, base[b]
    else:
        lane, pos = {(0, 1): 1, (1, 2): 2, (0, 2): 0}[(ii, kk)], base[b] + 1
    return 4 * (3 * (pos // 4) + lane) + pos % 4


def cov_words(P, compact):
    """[B, n, n] float64 -> the covariance words of a record as float64 [B, 120 or 48]: the symmetric part 0.5 * (P + P^T) formed in
    double, word sidx(a, b) holding element (a, b) of the 15 x 15 matrix (zero outside n x n), or for a compact record the row-major
    upper triangle of the 9 x 9 block followed by three zero padding words."""
    B, n = P.shape[:2]
    sym = 0.5 * (P + P.transpose(0, 2, 1))
    if compact:
        assert n == 9
        iu = np.triu_indices(9)
        return np.concatenate([sym[:, iu[0], iu[1]], np.zeros((B, 3))], axis=1)
    out = np.zeros((B, PW))
    order = sorted(sidx(a, b) for a in range(15) for b in range(a, 15))
    assert order == list(range(PW))
    for a in range(n):
        for b in range(a, n):
            out[:, sidx(a, b)] = sym[:, a, b]
    return out


def expected_pack(prior, B, dtype, compact, x=None, P=None, mask=None):
    """The record array (flat, of the compute dtype) after a pack of x [B,16] / P [B,n,n] (float64 values; None: kept) into `prior`."""
    T = NP_T[dtype]
    out = prior.copy()
    on = np.ones(B, bool) if mask is None else np.asarray(mask) != 0
    if x is not None:
        o = record_offsets(B, dtype, XW)
        out[o[on]] = x.astype(T)[on]
    if P is not None:
        cw = cov_words(P, compact).astype(T)
        o = XW + np.arange(cw.shape[1])
        o = off(o[None, :], np.arange(B)[:, None], dtype)
        out[o[on]] = cw[on]
    return out


def expected_copy(src, dst_prior, src_B, B, dtype, compact, index=None, mask=None, WT=SW, words=None):
    """(dst array after, written [B]): dst filter i <- src filter index[i] for mask != 0 and 0 <= index[i] < src_B, record words only."""
    words = RECORD_WORDS[compact] if words is None else words
    idx = np.arange(B, dtype=np.int64) if index is None else np.asarray(index, np.int64)
    ok = (idx >= 0) & (idx < src_B)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    out = dst_prior.copy()
    i = np.nonzero(ok)[0]
    w = np.arange(words)[None, :]
    out[off(w, i[:, None], dtype, WT)] = src[off(w, idx[i][:, None], dtype, WT)]
    return out, ok.astype(np.uint8)


_hip = None


def _runtime():
    """The HIP runtime the engine has already loaded into this process (found in the process's own mappings, not by a path)."""
    global _hip
    if _hip is None:
        import ctypes as C
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        _hip = C.CDLL(path)
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipDeviceSynchronize.argtypes = []
    return _hip


def raw_read(view):
    """Every word of the record array behind a `qle_device_view` (padded_batch x 144 words of its dtype, in array order), after the
    device has finished everything submitted to it."""
    T = np.float32 if view.dtype == 0 else np.float64
    out = np.empty(view.padded_batch * SW, T)
    hip = _runtime()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemcpy(out.ctypes.data, view.state, out.nbytes, 2) == 0    # hipMemcpyDeviceToHost
    return out


def raw_write(view, words):
    """Overwrite every word of the record array behind a view."""
    T = np.float32 if view.dtype == 0 else np.float64
    a = np.ascontiguousarray(words, T)
    assert a.size == view.padded_batch * SW
    hip = _runtime()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemcpy(view.state, a.ctypes.data, a.nbytes, 1) == 0        # hipMemcpyHostToDevice
    assert hip.hipDeviceSynchronize() == 0


def sentinel(B, dtype, seed, offset=0.0):
    """A record array for padded(B) filters in which every word is finite, non-zero and a multiple of 0.5 plus `offset`: two arrays
    drawn with offsets 0 and 0.25 differ in every word (all values are exact in float32)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 2 ** 20, padded(B) * SW) * 0.5 + 1000.0 + offset).astype(NP_T[dtype])


def random_state(B, n, seed, dtype="f64"):
    """x [B,16] with unit quaternions and P [B,n,n], NOT symmetric (the pack symmetrises), values of `dtype` held as float64"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, 16))
    x[:, 6:10] /= np.linalg.norm(x[:, 6:10], axis=1, keepdims=True)
    A = rng.normal(size=(B, n, n)) * 0.1
    P = A @ A.transpose(0, 2, 1) + 0.05 * np.eye(n) + 1e-3 * rng.normal(size=(B, n, n))
    T = NP_T[dtype]
    return x.astype(T).astype(np.float64), P.astype(T).astype(np.float64)
