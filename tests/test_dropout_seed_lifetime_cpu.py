"""``dropout.native_table`` hands the library the ADDRESS of the seed tensor: the table must keep the tensor alive, or a caller that
passes a temporary leaves the library reading memory the allocator has given to someone else (the masks then depend on what the
process allocated before).  No GPU."""
import gc
import weakref

import torch

from openviic_amd import dropout


def test_the_table_keeps_its_seed_tensor_alive():
    seed = torch.tensor([5], dtype=torch.int64)
    alive = weakref.ref(seed)
    address = seed.data_ptr()
    table = dropout.native_table({dropout.SITE_EMB: 0.1}, seed)
    del seed
    gc.collect()
    assert alive() is not None and table.seed == address and int(alive()[0]) == 5
    other = [torch.zeros(1, dtype=torch.int64) for _ in range(64)]           # none of these may land on the seed's memory
    assert all(t.data_ptr() != address for t in other)
    del table
    gc.collect()
    assert alive() is None
