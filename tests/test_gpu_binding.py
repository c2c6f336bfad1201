"""The binding helpers of moco_flow_amd/_lib.py on the device: launch / enqueue put the current stream
last and check the status under the symbol's name, scratch has one floor, and one real round trip through them -- a single
launch (gather_rows) and a multi-launch path with its host read (marching_cubes)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture
def L():
    import moco_flow_amd._lib as lib_module
    lib_module.lib()                                  # loaded before a test swaps it out
    return lib_module


class Stub:
    """Stands in for the loaded library: one entry point that records its arguments and the current device."""

    def __init__(self, rc=0, text=b"probe: the stub's message"):
        self.rc, self.text, self.calls = rc, text, []

    def probe(self, *args):
        self.calls.append((args, torch.cuda.current_device()))
        return self.rc

    def mf_last_error(self):
        return self.text


def test_launch_and_enqueue_pass_the_current_stream_last(L, monkeypatch):
    stub = Stub()
    monkeypatch.setattr(L, "_lib", stub)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", min(1, torch.cuda.device_count() - 1))      # not the current device where there are two
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        L.launch(dev, "probe", 1, 2)
        L.enqueue(dev, "probe", 1, 2)
    assert [c[0] for c in stub.calls] == [(1, 2, side.cuda_stream)] * 2
    assert stub.calls[0][1] == dev.index                            # launch ran it with dev current
    assert torch.cuda.current_device() == 0                         # and put the device back
    L.launch(dev, "probe")                                          # outside a stream context, from device 0
    L.enqueue(dev, "probe")
    assert [c[0] for c in stub.calls[2:]] == [(torch.cuda.current_stream(dev).cuda_stream,)] * 2
    assert stub.calls[2][1] == dev.index and stub.calls[3][1] == 0  # launch enters dev's context, enqueue enters none
    L.call("probe", 3)
    assert stub.calls[4][0] == (3,)                                 # call: no stream


@pytest.mark.parametrize("rc, kind", [(-3, NotImplementedError), (-1, RuntimeError)])
def test_a_failed_status_raises_under_the_symbols_name(L, monkeypatch, rc, kind):
    stub = Stub(rc=rc)
    monkeypatch.setattr(L, "_lib", stub)
    for fn in (L.launch, L.enqueue):
        with pytest.raises(kind) as e:
            fn(torch.device("cuda", 0), "probe", 1, 2)
        assert type(e.value) is kind and "probe" in str(e.value) and "the stub's message" in str(e.value)
    with pytest.raises(kind, match="the stub's message"):
        L.call("probe")
    with pytest.raises(kind, match="the stub's message"):
        L.need("probe", 5)


def test_scratch_has_one_floor(L):
    dev = torch.device("cuda", 0)
    assert L.need("mf_mask_compact_scratch_bytes", 0) == 0
    s = L.scratch(dev, "mf_mask_compact_scratch_bytes", 0)
    assert s.dtype == torch.uint8 and s.device == dev and s.numel() >= 16 and s.data_ptr() != 0
    big = L.need("mf_mask_compact_scratch_bytes", 1 << 20)
    assert big > 16 and L.scratch(dev, "mf_mask_compact_scratch_bytes", 1 << 20).numel() == big


def test_round_trip_single_launch_and_multi_launch_with_host_read():
    from moco_flow_amd import mesh
    src = torch.arange(12, dtype=torch.float32, device="cuda").view(4, 3)
    inds = torch.tensor([3, 0], dtype=torch.int64, device="cuda")
    assert torch.equal(mesh.gather_rows(src, inds), src[[3, 0]])
    volume = torch.ones((2, 2, 2), dtype=torch.float32, device="cuda")
    volume[0, 0, 0] = 0.0                                            # one corner below the isovalue: one triangle
    verts, tris = mesh.marching_cubes(volume, 0.5)
    assert tuple(verts.shape) == (3, 3) and tuple(tris.shape) == (1, 3)
    assert sorted(tris[0].tolist()) == [0, 1, 2]
    want = torch.tensor([[0.0, 0.0, 0.5], [0.0, 0.5, 0.0], [0.5, 0.0, 0.0]])      # the three edges at that corner, halfway
    assert torch.equal(verts.cpu()[torch.argsort(verts.cpu() @ torch.tensor([4.0, 2.0, 1.0]))], want)
