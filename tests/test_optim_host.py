"""CPU (-m "not gpu"): the host side of generativemodels_amd.optim -- the constructor's validation against torch.optim's, the param-group keys, the refusals
of step() that need no device (dtype pairing, CPU tensors, sparse and non-dense gradients), the chunk planner, and the state-dict layout through
torch.optim.Adam.load_state_dict on host tensors.  No kernel runs here."""
import itertools

import pytest
import torch

import generativemodels_amd as gm
from generativemodels_amd import optim

SIZES = (1, 3, 5, 1023, 4097, 65537)
PAIRS = ((optim.Adam, torch.optim.Adam), (optim.AdamW, torch.optim.AdamW))


def _params(dtype=torch.float32):
    g = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(n, generator=g).to(dtype)) for n in SIZES]


def test_exported_as_gm_optim():
    assert gm.optim is optim and issubclass(optim.AdamW, optim.Adam) and issubclass(optim.Adam, torch.optim.Optimizer)


@pytest.mark.parametrize("bad", [dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(-0.1, 0.999)), dict(betas=(0.9, 1.0)),
                                 dict(betas=(0.9, -0.5)), dict(weight_decay=-0.1), dict(betas=(0, 0.999)), dict(lr=torch.ones(2))],
                         ids=lambda b: "-".join(f"{k}" for k in b) + "-" + str(abs(hash(str(b))) % 1000))
@pytest.mark.parametrize("mine,theirs", PAIRS, ids=("Adam", "AdamW"))
def test_constructor_refuses_what_torch_refuses_with_the_same_exception(mine, theirs, bad):
    with pytest.raises(Exception) as want:
        theirs(_params(), **bad)
    with pytest.raises(Exception) as got:
        mine(_params(), **bad)
    assert type(got.value) is type(want.value) is ValueError
    assert str(got.value) == str(want.value)


def test_empty_parameter_list_and_duplicate_parameters_are_torchs_errors():
    for mine, theirs in PAIRS:
        with pytest.raises(ValueError, match="empty parameter list"):
            theirs([])
        with pytest.raises(ValueError, match="empty parameter list"):
            mine([])
        p = _params()
        with pytest.raises(ValueError, match="more than one parameter group"):
            mine([{"params": p}, {"params": p[:1]}])


@pytest.mark.parametrize("mine,theirs", PAIRS, ids=("Adam", "AdamW"))
def test_defaults_and_param_group_keys_are_torchs(mine, theirs):
    a, b = mine(_params()), theirs(_params())
    assert list(a.param_groups[0].keys()) == list(b.param_groups[0].keys())
    for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "decoupled_weight_decay"):
        assert a.param_groups[0][k] == b.param_groups[0][k], k
    p = _params()
    o = mine([{"params": p[:2], "lr": 0.5, "weight_decay": 0.25}, {"params": p[2:], "betas": (0.5, 0.75)}], lr=0.125, amsgrad=True)
    assert [g["lr"] for g in o.param_groups] == [0.5, 0.125] and o.param_groups[0]["weight_decay"] == 0.25
    assert o.param_groups[1]["betas"] == (0.5, 0.75) and all(g["amsgrad"] for g in o.param_groups)
    assert o.state_dict()["state"] == {}  # no gradient yet: no state


def test_cpu_parameters_are_refused_at_step():
    p = _params()
    opt = optim.Adam(p, lr=1e-2)
    opt.step()  # no gradient anywhere: nothing to do, as in torch
    assert len(opt.state) == 0
    for q in p:
        q.grad = torch.ones_like(q)
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        opt.step()
    opt.zero_grad()
    assert all(q.grad is None for q in p)


def test_mixed_dtype_pairs_name_the_parameter():
    p = _params()
    opt = optim.Adam(p)
    p[3].grad_dtype = None  # (torch itself refuses a gradient of another dtype unless the parameter says it takes any)
    p[3].grad = torch.ones(SIZES[3], dtype=torch.bfloat16)
    with pytest.raises(TypeError, match=r"parameter 3 of param group 0 \(shape \(1023,\)\).*float32.*bfloat16"):
        opt.step()
    named = torch.nn.Linear(3, 2).bfloat16()
    opt = optim.AdamW(named.named_parameters())
    named.bias.grad_dtype = None
    named.bias.grad = torch.ones(2)
    with pytest.raises(TypeError, match="parameter 'bias'"):
        opt.step()
    half = [torch.nn.Parameter(torch.ones(4, dtype=torch.float16))]
    half[0].grad = torch.ones(4, dtype=torch.float16)
    with pytest.raises(TypeError, match="parameter 0 of param group 0"):
        optim.Adam(half).step()


def test_sparse_and_non_dense_gradients():
    p = [torch.nn.Parameter(torch.ones(4, 4))]
    p[0].grad = torch.ones(4, 4).to_sparse()
    with pytest.raises(RuntimeError, match="does not support sparse gradients"):
        optim.Adam(p).step()
    p[0].grad = torch.ones(4, 8)[:, ::2]
    with pytest.raises(ValueError, match=r"parameter 0 of param group 0 \(shape \(4, 4\)\).*not dense"):
        optim.Adam(p).step()
    q = [torch.nn.Parameter(torch.ones(8, 4)[::2])]
    q[0].grad = torch.ones(4, 4)
    with pytest.raises(ValueError, match="not dense"):
        optim.Adam(q).step()


# ---- the planner ---------------------------------------------------------------------------------------------------------------------------------------
OFFSETS = (0, 4, 8)


def _addresses(n_ptrs, offsets):
    return [4096 * (k + 1) + off for k, off in zip(range(n_ptrs), offsets)]


@pytest.mark.parametrize("n_ptrs", (4, 5))
def test_planner_covers_every_element_once_and_vectorises_only_aligned_chunks(n_ptrs):
    for g_off, m_off in itertools.product(OFFSETS, OFFSETS):
        offs = [(0, g_off, m_off, 0, 0)[:n_ptrs]] * len(SIZES)
        addr = [_addresses(n_ptrs, o) for o in offs]
        chunks = optim.plan_chunks(SIZES, addr)
        for i, n in enumerate(SIZES):
            mine = [c for c in chunks if c.tensor == i]
            seen = torch.zeros(n, dtype=torch.int32)
            for c in mine:
                assert 0 < c.count <= optim.CHUNK and c.start % 8 == 0
                seen[c.start:c.start + c.count] += 1
                aligned = all((a + c.start * 4) % 16 == 0 for a in addr[i])  # the chunk's own pointers (4-byte elements)
                assert c.vec == aligned and (not c.vec or (g_off == 0 and m_off == 0))
            assert bool((seen == 1).all()), (n, g_off, m_off)
        assert len(chunks) == sum(-(-n // optim.CHUNK) for n in SIZES)


def test_planner_chunk_count_is_independent_of_tensor_order_and_of_alignment():
    base = None
    for perm in itertools.permutations(range(len(SIZES)), len(SIZES)):
        if perm[0] > 1:  # (a sixth of the 720 orders is plenty)
            continue
        sizes = [SIZES[i] for i in perm]
        for off in OFFSETS:
            chunks = optim.plan_chunks(sizes, [_addresses(4, (0, off, 0, 0))] * len(sizes), chunk=1024)
            count = len(chunks)
            base = count if base is None else base
            assert count == base == sum(-(-n // 1024) for n in SIZES)
            assert sorted((sizes[c.tensor], c.start, c.count) for c in chunks) == sorted(
                (n, s, min(1024, n - s)) for n in SIZES for s in range(0, n, 1024))
    with pytest.raises(ValueError):
        optim.plan_chunks([8], [[0]], chunk=12)


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------------------------------
def _torch_steps(opt, params, steps, seed):
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()


@pytest.mark.parametrize("mine,theirs,kw", [(optim.Adam, torch.optim.Adam, {}), (optim.AdamW, torch.optim.AdamW, dict(amsgrad=True, weight_decay=0.1))],
                         ids=("Adam", "AdamW-amsgrad"))
def test_state_dict_round_trips_through_torch_on_host_tensors(mine, theirs, kw):
    p_ref, p_a, p_b = _params(), _params(), _params()
    ref = theirs(p_ref, lr=1e-2, **kw)
    _torch_steps(ref, p_ref, 5, seed=1)

    a = theirs(p_a, lr=1e-2, **kw)
    _torch_steps(a, p_a, 3, seed=1)
    sd = a.state_dict()
    here = mine(p_a, lr=0.5)  # (the checkpoint's groups win, as in torch)
    here.load_state_dict(sd)
    back = here.state_dict()
    assert back["param_groups"] == sd["param_groups"]
    assert set(back["state"]) == set(sd["state"]) == set(range(len(SIZES)))
    for k, st in sd["state"].items():
        assert set(back["state"][k]) == set(st) == {"step", "exp_avg", "exp_avg_sq"} | ({"max_exp_avg_sq"} if kw else set())
        for name, v in st.items():
            got = back["state"][k][name]
            assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.shape == v.shape and torch.equal(got, v.float()), (k, name)
    # the counters are elements of one flat buffer here, and tensors of their own in the checkpoint
    assert all(here.state[q]["step"].item() == 3.0 for q in p_a)
    assert back["state"][0]["step"].data_ptr() != here.state[p_a[0]]["step"].data_ptr()

    # ... and what was written here resumes in torch: two more steps there equal five uninterrupted ones
    for q, r in zip(p_b, p_a):
        q.data.copy_(r.data)
    b = torch.optim.Adam(p_b, lr=0.5)  # (Adam takes AdamW's groups: decoupled_weight_decay travels in them)
    b.load_state_dict(back)
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        for q in p_b:
            torch.randn(q.shape, generator=g)
    for _ in range(2):
        for q in p_b:
            q.grad = torch.randn(q.shape, generator=g)
        b.step()
    for q, r in zip(p_b, p_ref):
        assert torch.equal(q, r)
    for q, r in zip(p_b, p_ref):
        for name in b.state[q]:
            assert torch.equal(torch.as_tensor(b.state[q][name]), torch.as_tensor(ref.state[r][name])), name


def test_load_state_dict_takes_plain_number_steps_and_keeps_fp32_moments_of_bf16_parameters():
    p = [torch.nn.Parameter(torch.ones(5, dtype=torch.bfloat16))]
    sd = {"state": {0: {"step": 7, "exp_avg": torch.full((5,), 1.0 + 2.0 ** -20), "exp_avg_sq": torch.full((5,), 3.0)}},
          "param_groups": [dict(optim.Adam(p).param_groups[0], params=[0])]}
    opt = optim.Adam(p)
    opt.load_state_dict(sd)
    st = opt.state[p[0]]
    assert st["step"].item() == 7.0 and st["step"].dtype == torch.float32
    assert st["exp_avg"].dtype == torch.float32 and torch.equal(st["exp_avg"], sd["state"][0]["exp_avg"])  # (bf16 would round it to 1.0)
    keep = st["exp_avg_sq"]
    sd["state"][0]["exp_avg_sq"] = torch.full((5,), 4.0)
    opt.load_state_dict(sd)  # existing state is refilled in place: a captured graph holds its address
    assert opt.state[p[0]]["exp_avg_sq"].data_ptr() == keep.data_ptr() and keep[0].item() == 4.0
