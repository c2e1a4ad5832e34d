"""`records.transitions` on synthetic record blocks, numpy and torch (CPU): the replay tuples of a closed-loop block.  `obs`
is shifted by one step, `next_obs` comes from the terminal tail exactly where terminated | truncated, the NaN tails of
unfinished rows never reach the result, and what can be a view of the block is one.  No GPU needed."""
import numpy as np
import pytest

from underwater_swimmer_rl_amd.records import REC_EXTRA_COLS, pack_record, record_width, transitions, unpack_record

H, N, D, A = 5, 7, 24, 2


def synthetic(seed=0):
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((H, N, D)).astype(np.float32)
    reward = rng.standard_normal((H, N)).astype(np.float32)
    term = rng.random((H, N)) < 0.25
    trunc = (rng.random((H, N)) < 0.25) & ~term
    term[0, 0], trunc[0, 0] = True, True          # both flags in one row: still one finished row
    term[1, 1], trunc[1, 1] = False, False
    term[2, 2], trunc[2, 2] = True, False
    term[3, 3], trunc[3, 3] = False, True
    info = rng.integers(0, 50, (H, N, 3)).astype(np.int32)
    final = rng.standard_normal((H, N, D)).astype(np.float32)
    done = term | trunc
    final[~done] = np.nan                           # what the kernels leave in a NaN-filled block
    rec = pack_record(obs, reward, term, trunc, info, final)
    first = rng.standard_normal((N, D)).astype(np.float32)
    actions = rng.standard_normal((H, N, A)).astype(np.float32)
    return rec, first, actions, obs, reward, term, trunc, final


def check(result, first, actions, obs, reward, term, trunc, final, to_numpy):
    o, a, r, nx, te = (to_numpy(x) for x in result)
    assert o.shape == (H * N, D) and a.shape == (H * N, A) and r.shape == (H * N,) and nx.shape == (H * N, D) and te.shape == (H * N,)
    o, nx = o.reshape(H, N, D), nx.reshape(H, N, D)
    assert np.array_equal(o[0], first) and np.array_equal(o[1:], obs[:-1])         # the row each action saw
    done = term | trunc
    assert done.any() and (~done).any() and (term & ~trunc).any() and (trunc & ~term).any()
    assert np.array_equal(nx[done], final[done]) and np.array_equal(nx[~done], obs[~done])
    assert not np.isnan(nx).any()
    assert np.array_equal(a.reshape(H, N, A), actions) and np.array_equal(r.reshape(H, N), reward)
    assert te.dtype == np.bool_ and np.array_equal(te.reshape(H, N), term)           # truncation alone is not termination


def test_numpy_block():
    rec, first, actions, obs, reward, term, trunc, final = synthetic()
    before = rec.copy()
    out = transitions(first, rec, actions, D)
    check(out, first, actions, obs, reward, term, trunc, final, np.asarray)
    assert np.array_equal(rec.view(np.uint32), before.view(np.uint32))               # the block is only read
    o, a, r, nx, te = out
    assert np.shares_memory(r, rec) and np.shares_memory(te, rec) and np.shares_memory(a, actions)
    assert not np.shares_memory(o, rec) and not np.shares_memory(nx, rec)            # shifted / selected: new blocks


def test_torch_cpu_block():
    torch = pytest.importorskip("torch")
    rec, first, actions, obs, reward, term, trunc, final = synthetic(1)
    t_rec, t_first, t_act = torch.from_numpy(rec.copy()), torch.from_numpy(first), torch.from_numpy(actions)
    out = transitions(t_first, t_rec, t_act, D)
    assert all(isinstance(x, torch.Tensor) for x in out)
    check(out, first, actions, obs, reward, term, trunc, final, lambda x: x.numpy())
    o, a, r, nx, te = out
    base = t_rec.untyped_storage().data_ptr()
    assert r.untyped_storage().data_ptr() == base and te.untyped_storage().data_ptr() == base
    assert a.untyped_storage().data_ptr() == t_act.untyped_storage().data_ptr()
    assert te.dtype == torch.bool


def test_nan_tails_do_not_leak_even_where_obs_is_zero():
    """A product with a mask (done * final + (1 - done) * obs) would turn NaN * 0 into NaN: the rows are selected."""
    rec, first, actions, obs, reward, term, trunc, final = synthetic(2)
    u = unpack_record(rec, D)
    u["obs"][...] = 0.0
    nx = transitions(first, rec, actions, D)[3].reshape(H, N, D)
    done = term | trunc
    assert np.isnan(final[~done]).all() and not np.isnan(nx).any() and (nx[~done] == 0.0).all()


def test_blocks_that_do_not_fit_are_refused():
    rec, first, actions, *_ = synthetic()
    narrow = np.ascontiguousarray(rec[..., :record_width(D, False)])
    assert narrow.shape[-1] == D + REC_EXTRA_COLS
    with pytest.raises(ValueError, match="terminal observation"):
        transitions(first, narrow, actions, D)
    with pytest.raises(ValueError):
        transitions(first[:-1], rec, actions, D)
    with pytest.raises(ValueError):
        transitions(first, rec, actions[:-1], D)
    with pytest.raises(ValueError):
        transitions(first, rec[0], actions[0], D)
    with pytest.raises(ValueError):
        transitions(first, rec, actions, D + 1)
