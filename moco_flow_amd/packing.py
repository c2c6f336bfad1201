"""Packed-weights cache: nn.Linear tensors -> the kernels' MFMA fragment stream.

The packed buffer is rebuilt whenever any parameter's storage pointer or version
counter changes (optimizer.step, load_state_dict, .to(device)).  Edits made THROUGH ``param.data``
(``p.data.mul_()``, ``p.data.copy_()``: EMA / manual-init idioms) bump no version counter: call
``module.invalidate_packed()`` (NeRF / NoF) after them.

The cache holds ctypes structures with raw device pointers, which must not travel: pickling
(``torch.save(model)``) and ``copy.deepcopy(model)`` drop it and the copy re-packs on first use.

Streams and threads.  The pack kernel runs on the stream that was current when the cache was (re)built, and the caller
cannot see that it ran.  So the cache remembers that stream (``BuildOrder``): a call under another current stream makes
its stream wait for the build -- once per (build, consumer stream) -- before it hands the buffer out; a call under the
build's own stream pays one integer compare: no event, no launch, no host synchronisation.  While the current stream is
capturing a graph nothing is added: the caller's ``wait_stream`` in front of the capture orders the warm-up's pack, as
torch requires of every capture.  What a build leaves behind is published as ONE object in one attribute store, and ``get``
answers from the object it read: a second thread sees the old (key, desc, buf, keep) or the new one, never a mix.  The
old buffer is freed when the weights changed; a caller who changes weights that another stream still reads has broken
torch's own rule (as with nn.Linear), and nothing here repairs that."""
import torch

from . import _lib as L


def _collect_params(m, out):
    for p in m._parameters.values():
        if p is not None:
            out.append(p)
    for c in m._modules.values():
        if c is not None:
            _collect_params(c, out)


class BuildOrder:
    """The stream a hidden device cache was filled on, and the streams that already wait for that fill.
    ``order(dev)`` in front of every hand-out of the cached memory."""
    __slots__ = ("stream", "stream_id", "event", "waited")

    def __init__(self, dev):
        self.stream = torch.cuda.current_stream(dev)      # kept: its handle cannot come back under another stream
        self.stream_id = self.stream.cuda_stream
        self.event = None
        self.waited = set()

    def order(self, dev):
        cur = torch.cuda.current_stream(dev)
        if cur.cuda_stream != self.stream_id:
            _order_foreign(self, cur)


def _order_foreign(o, cur):
    """``cur`` is not the build's stream: make it wait for the build, once.  The event is recorded here, at the first
    foreign consumer, on the build stream's tail -- behind the fill, and behind a little more than necessary."""
    if cur.cuda_stream in o.waited or torch.cuda.is_current_stream_capturing():
        return
    if o.event is None:
        ev = torch.cuda.Event()
        ev.record(o.stream)
        o.event = ev
    cur.wait_event(o.event)
    o.waited.add(cur.cuda_stream)


_EMPTY = (None, None, None, None, None)       # (key, desc, buf, keep, order)


class PackedWeights:
    def __init__(self):
        self.state = _EMPTY

    key = property(lambda self: self.state[0])
    desc = property(lambda self: self.state[1])
    buf = property(lambda self: self.state[2])
    keep = property(lambda self: self.state[3])   # contiguous fp32 views the descriptor points into

    def invalidate(self):
        self.state = _EMPTY

    def __getstate__(self):          # torch.save(module) / pickle: nothing cached travels
        return {}

    def __setstate__(self, state):
        self.invalidate()

    def __deepcopy__(self, memo):    # copy.deepcopy(module): the copy packs its own parameters
        return PackedWeights()

    def get(self, module, build_desc, bytes_fn, pack_fn, what, precision=0):
        # (module.parameters() builds names and de-duplicates through sets on every call: ~50 us per network and render
        #  pass, a tenth of a bf16 pass; this plain walk of the module tree reads the same tensors in the same order in ~10 us
        #  and still sees replaced parameters and sub-modules)
        params = []
        _collect_params(module, params)
        if not params:
            raise RuntimeError(f"{what}: module has no parameters")
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError(f"moco_flow_amd.{what}: parameters are on '{dev}'. This is the MI355X (HIP) "
                               "path; there is no CPU implementation. Call .to('cuda') first.")
        key = (precision,) + tuple((p.data_ptr(), p._version, p.dtype) for p in params)
        st = self.state                                  # one read: everything below comes from this object
        if key != st[0]:
            desc, keep = build_desc()
            nbytes = bytes_fn(desc, precision)
            if nbytes <= 0:                              # a negative size is the library's code; 0 is how the *_packed_bytes
                L.check(nbytes or -3, what)              # queries say "unsupported configuration" (MF_E_UNSUPPORTED)
            buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                order = BuildOrder(dev)
                L.check(pack_fn(desc, precision, buf.data_ptr(), order.stream_id), what + " pack")
            self.state = st = (key, desc, buf, keep, order)      # one store, after the launch
        else:
            st[4].order(dev)
        return st[1], st[2]
