"""What the GPU tests share that touches torch or an engine context: device tensors, guard rows, the K2 kernel names and plans, and
the module fixtures.  A plain module like edge_words.py: imported by name, not collected; torch is imported inside the functions, so
collecting the suite needs no torch.

A context runs on a non-blocking stream of its own, which does not wait for work torch queued on its stream.  So every tensor made
here is settled -- torch's stream synchronised -- before it is returned: a sentinel fill cannot land after the kernel's stores, a
guard row cannot be read before its fill, an upload cannot still be in flight when the engine reads it.

The fixtures are module-scoped and imported by the test files that use them (`from gpu_support import toy_server, tc  # noqa: F401`):
every module has its own Server, so its own key upload, and its own client, so its own sequence of encryptions."""
import numpy as np
import pytest

from aes_vectors import F5, own_client

SENTINEL = -0x5A5A5A5A5A5A5A5B      # an int64 bit pattern no kernel is asked to write
GUARD = 2

LATENCY = "blind_rotate_latency_kernel<5,5,8>"
HOME = "blind_rotate16_kernel<5,5,8,3,2,true>"
PARKED = "blind_rotate16_kernel<5,5,8,3,2,false>"
PAIR = "blind_rotate_pair_kernel<5,5,8,3,2>"
FORMS = {"default": (True, True), "pair denied": (False, True), "home denied": (True, False), "both denied": (False, False)}


# ---- device tensors ----------------------------------------------------------------------------------------------------------------
def settled(t):
    """t, once everything queued on torch's stream is done: a context runs on a non-blocking stream of its own, which does not wait for
    the fill, copy or gather that made one of its arguments"""
    import torch

    torch.cuda.synchronize()
    return t


def dev(a):
    """a host array of 64-bit words as an int64 tensor on the GPU"""
    import torch

    return settled(torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda())


def host(t):
    """a device tensor of 64-bit words as a uint64 array"""
    return t.cpu().numpy().view(np.uint64)


def filled(shape, value):
    import torch

    return settled(torch.full(tuple(shape), value, dtype=torch.int64, device="cuda"))


def guarded(rows, words):
    """(a sentinel-filled device tensor of rows + 2 GUARD rows, its middle `rows` rows)"""
    buf = filled((rows + 2 * GUARD, words), SENTINEL)
    return buf, buf[GUARD:GUARD + rows]


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all().item()) and bool((buf[-GUARD:] == SENTINEL).all().item())


# ---- K2 plans ----------------------------------------------------------------------------------------------------------------------
def plan_tuple(pl):
    return (pl["form"], pl["units_main"], pl["r_main"], pl["units_tail"], pl["r_tail"])


def unit_rows(plan, u, m):
    """the valid rows of unit u in a launch of m rows, a ragged unit's empty slots left out; plan as k2_plan gives it or as plan_tuple"""
    _, um, rm, _, rt = plan_tuple(plan) if isinstance(plan, dict) else plan
    lo = u * rm if u < um else um * rm + (u - um) * rt
    return list(range(lo, min(lo + (rm if u < um else rt), m)))


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy_server(toy):
    from tfhe_aes_amd.server import Server

    return Server(toy.keys, device=0, engine=toy.engine())


@pytest.fixture(scope="module")
def opt_server(opt):
    from tfhe_aes_amd.server import Server

    return Server(opt.keys, device=0, engine=opt.engine())


@pytest.fixture(scope="module")
def tc(toy):
    return own_client(toy)


@pytest.fixture(scope="module")
def oc(opt):
    return own_client(opt)


@pytest.fixture(scope="module")
def opt_rk128(opt_server, oc):
    """resident round keys of the SP 800-38A F.1.1 key, expanded on the GPU"""
    d_ek = dev(oc.encrypt_aes_key(F5[128][0]))
    d_rk = opt_server.aes_key_expansion(d_ek)
    opt_server.synchronize()
    return d_rk
