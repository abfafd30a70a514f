"""The key of the per-stream scratch caches (_native.stream_key, _native.PerStream): torch.device("cuda") and
torch.device("cuda", current_device()) are the same device, so what one spelling created the other one finds — the ordering
flag of uoc_roi_match that _finish_block has to see included."""
import pytest
import torch

from unseenobjectclustering_amd import _native
from unseenobjectclustering_amd.fcn import test_dataset as TD

pytestmark = pytest.mark.gpu


def test_a_device_without_an_index_is_the_current_one(device):
    cur = torch.cuda.current_device()
    bare, full = torch.device("cuda"), torch.device("cuda", cur)
    assert _native.stream_key(bare) == _native.stream_key(full) == ("cuda", cur, int(torch.cuda.current_stream(full).cuda_stream))
    status = TD._status_word(bare)                       # the stream's status word, created (or found) under one spelling ...
    assert status.shape == (1,) and status.dtype == torch.int32
    status.zero_()
    assert TD._status_word(full) is status               # ... is the one the other spelling finds
    for raised_under, seen_under in ((bare, full), (full, bare), (bare, bare), (full, full)):
        TD._status_word(raised_under).fill_(1)
        with pytest.raises(TD.HostOrderNeeded):
            TD._finish_block(seen_under)
        assert int(status.item()) == 0                   # read and cleared
        TD._finish_block(seen_under)                     # nothing left to report
    main_key, side = _native.stream_key(full), torch.cuda.Stream(full)
    with torch.cuda.stream(side):                        # another stream of the same device: its own word, the same device
        assert _native.stream_key(bare) == _native.stream_key(full) != main_key
        other = TD._status_word(bare)
        assert other is not status and TD._status_word(full) is other
        other.fill_(1)
    torch.cuda.synchronize(full)
    with pytest.raises(TD.HostOrderNeeded):
        TD._finish_block(bare)                           # every stream of the device is asked
    assert int(other.item()) == 0 and int(status.item()) == 0
