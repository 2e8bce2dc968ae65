"""The tensor arguments of the device-resident entry points, in one place: what a valid device tensor is (dev), how a tensor
becomes the pointer the C entry takes (ptr / ptr_array / ptr_opt), how the outputs of a call are allocated in the order of its C
arguments (alloc), and the groups of arguments that recur (keypoints, pair_arrays, pinhole, defaults).  It knows neither
hip.py nor the library: torch tensors are only the device buffers."""
import ctypes as C

# An empty tensor has no storage: its pointer is 0.  The entries that take their arrays even when they hold nothing read a 0 as
# NULL, "not given", and refuse the call; such an array goes in as this address, which is never dereferenced (no element exists).
_EMPTY_ARRAY = 256


def dev(name, t, dtype, numel=None, *, optional=False, multiple_of=None):
    """t, when it is what a kernel may take as a raw pointer: a contiguous cuda tensor of `dtype` (the name of a torch dtype:
    "int32"; a wrapper that only names dtypes need not import torch), with `numel` elements (if given) or a multiple of
    `multiple_of` (if given).  None passes only when optional.  Anything else raises ValueError with the argument's name -- an
    exception, not an assert: these are checks on input from outside and must survive python -O."""
    if t is None:
        if optional:
            return None
        raise ValueError("%s: a device tensor is required, got None" % name)
    if not t.is_cuda:
        raise ValueError("%s: not a cuda tensor (device %s)" % (name, t.device))
    if str(t.dtype) != "torch." + dtype:
        raise ValueError("%s: dtype %s, expected torch.%s" % (name, t.dtype, dtype))
    if not t.is_contiguous():
        raise ValueError("%s: not contiguous (shape %s, strides %s)" % (name, tuple(t.shape), tuple(t.stride())))
    if numel is not None and t.numel() != numel:
        raise ValueError("%s: %d elements (shape %s), expected %d" % (name, t.numel(), tuple(t.shape), numel))
    if multiple_of is not None and t.numel() % multiple_of != 0:
        raise ValueError("%s: %d elements (shape %s), expected a multiple of %d" % (name, t.numel(), tuple(t.shape), multiple_of))
    return t


def require(ok, what):
    """A relation between arguments that no single dev() states."""
    if not ok:
        raise ValueError(what)


def ptr(t):
    """None -> NULL; a tensor -> its pointer, 0 when it is empty."""
    return None if t is None else C.c_void_p(t.data_ptr())


def ptr_array(t):
    """An array the entry wants even when it holds nothing: an empty tensor goes in as a dummy address, None is refused."""
    if t is None:
        raise ValueError("an array argument that must be given is None")
    return C.c_void_p(t.data_ptr() or _EMPTY_ARRAY)


def ptr_opt(t):
    """None -> NULL, "not given"; a tensor as ptr_array, so that an empty one still counts as given."""
    return None if t is None else ptr_array(t)


def alloc(device, spec):
    """The outputs of a call: spec maps name -> (shape, dtype name) or (shape, dtype name, True) for a zeroed tensor, in the
    order of the C arguments; an entry that is None (an output that was not asked for) or already a tensor (an output in place)
    stays as it is.  -> dict in the order of spec."""
    import torch
    out = {}
    for name, v in spec.items():
        if isinstance(v, tuple):
            make = torch.zeros if len(v) > 2 and v[2] else torch.empty
            v = make(v[0], dtype=getattr(torch, v[1]), device=device)
        out[name] = v
    return out


def keypoints(kps):
    """kps: the F x cap x 7 float32 view of the KeyPoint records -> (F, cap)."""
    dev("kps", kps, "float32")
    require(kps.dim() == 3 and kps.shape[2] == 7, "kps: shape %s, expected F x cap x 7" % (tuple(kps.shape),))
    return kps.shape[0], kps.shape[1]


def pair_arrays(counts, F, cap, pair_q, pair_t, idx1, mask=None, mask_name="keep"):
    """The key-frame / pair arrays of the pair and map entries: counts F int32, pair_q / pair_t P int32, idx1 P x cap int32,
    mask P x cap uint8 or None -> P."""
    dev("counts", counts, "int32", F)
    dev("pair_q", pair_q, "int32")
    dev("pair_t", pair_t, "int32")
    P = pair_q.shape[0]
    require(pair_t.shape[0] == P, "pair_t: %d pairs, pair_q has %d" % (pair_t.shape[0], P))
    dev("idx1", idx1, "int32", P * cap)
    dev(mask_name, mask, "uint8", P * cap, optional=True)
    return P


def pinhole(k):
    """(fx, fy, cx, cy) as the four doubles of the C arguments."""
    fx, fy, cx, cy = (float(v) for v in k)
    return C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy)


def defaults(params, Struct, fn):
    """params, or a Struct that the library's fn(&struct) has filled with its defaults."""
    if params is not None:
        return params
    p = Struct()
    fn(C.byref(p))
    return p
