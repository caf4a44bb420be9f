"""The rollout's packed-mask cache (rollout._MaskCache) must not hand out the bits of a freed mask to a new tensor
that happens to sit at the same address with the same version counter and shape -- what a module built after another
was freed gets from the caching allocator (same id(), same key).  The device bit-packing is replaced by a copy so the
test runs on the host; two tensors over one numpy buffer give the same address deterministically."""
import gc

import numpy as np
import torch

from prob_mbrl_amd import rollout as RO


def test_mask_cache_misses_on_a_new_tensor_at_a_freed_address(monkeypatch):
    monkeypatch.setattr(RO.E, 'pack_mask', lambda m: m.clone())
    cache = RO._MaskCache()
    key = (12345, 'd', 0)
    buf = np.zeros((40, 32), dtype=np.float32)
    old = torch.from_numpy(buf)
    assert torch.equal(cache.get(key, old, 40), torch.zeros(40, 32))
    ptr, ver = old.data_ptr(), old._version
    del old
    gc.collect()
    buf[:] = 1.0                            # another module's mask, written without a torch op
    new = torch.from_numpy(buf)
    assert (new.data_ptr(), new._version) == (ptr, ver)
    assert torch.equal(cache.get(key, new, 40), torch.ones(40, 32))
    # the same live tensor is still served from the cache, and a change through torch still misses
    assert cache.get(key, new, 40) is cache.get(key, new, 40)
    new.mul_(0.0)
    assert torch.equal(cache.get(key, new, 40), torch.zeros(40, 32))
