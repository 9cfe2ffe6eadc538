"""CPU checks added in round 6: host-side support predicate of the listed weight-gradient launches."""
from realise_amd import _capi


def test_live_block_list_lds_is_sized_from_the_batch():
    """the live-block list of a listed TN launch sits in LDS: 4 KB (the bench shape, two 64 KB workgroups per CU) up to 16 KB = 4096
    blocks = 65536 bf16 token rows; longer lists are refused (the engine then builds no liveness tables: dense reductions)."""
    lib = _capi.load()
    f = lib.realise_debug_tn_list_lds
    assert f(1) == 4096 and f(512) == 4096 and f(1024) == 4096
    assert f(1025) == 5120 and f(2048) == 8192 and f(4096) == 16384
    assert f(4097) == -1 and f(1 << 20) == -1
