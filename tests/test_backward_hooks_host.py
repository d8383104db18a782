"""Host: ops.at_end_of_backward, the one place where end-of-backward work is queued (side-stream join, lane join, grouped
weight gradients, the early stage's buffers, the grad sinks' check).  CPU tensors and small autograd Functions: the helper
knows nothing of the GPU.  What it promises: once per (key, pass); again in the next pass — also when the pass before
raised, in which case the engine dropped the callback and the caller can see that nothing is queued for its key; outside a
pass either now or not at all; a reentrant pass is a pass of its own; no mark outlives its pass, and the mark a failed
pass left goes with its key."""
import gc

import pytest
import torch

from unscene3d_amd import ops


class _Key:
    """What the marks are kept for: some object of the caller's (held weakly)."""


A, B = _Key(), _Key()


class _Hooked(torch.autograd.Function):
    """Identity whose backward runs `body()` inside the backward pass."""

    @staticmethod
    def forward(ctx, x, body):
        ctx.body = body
        return x * 1.0

    @staticmethod
    def backward(ctx, g):
        ctx.body()
        return g, None


class _Poison(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x * 1.0

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError("poisoned backward node")


def _pass(body, poison=False):
    """One backward pass whose only hooked node runs `body`; poison: a node that runs AFTER it raises."""
    w = torch.ones(3, requires_grad=True)
    x = _Poison.apply(w) if poison else w          # created first -> lower sequence number -> runs later
    _Hooked.apply(x, body).sum().backward()


@pytest.fixture(autouse=True)
def _no_marks_left():
    assert not ops._END_MARKS
    yield
    assert not ops._END_MARKS, "a mark outlived its backward pass"


def test_once_per_key_and_pass_and_again_in_the_next_pass():
    ran, tasks = [], []

    def body():
        tasks.append(ops._graph_task())
        before = list(ran)
        assert not ops.queued_at_end_of_backward(A)
        ops.at_end_of_backward(A, lambda: ran.append("a"), outside="skip")
        assert ops.queued_at_end_of_backward(A) and not ops.queued_at_end_of_backward(B)
        ops.at_end_of_backward(A, lambda: ran.append("a again"), outside="skip")
        ops.at_end_of_backward(B, lambda: ran.append("b"), outside="run")
        assert ran == before, "the callbacks run when the pass ends, not before"
    _pass(body)
    assert ran == ["a", "b"] and tasks[0] >= 0
    _pass(body)
    assert ran == ["a", "b", "a", "b"] and tasks[1] != tasks[0]


def test_a_pass_that_raised_does_not_keep_the_next_one_from_queueing():
    ran, stale, others = [], [], []

    def body():
        # what a caller with state of its own asks (units._WgradQueue): a mark and nothing queued -> left by a dead pass
        stale.append(A in ops._END_MARKS and not ops.queued_at_end_of_backward(A))
        ops.at_end_of_backward(A, lambda: ran.append("a"), outside="skip")
        others.append(_Key())                       # a key that lives as long as its pass's state: a GradSink
        ops.at_end_of_backward(others[-1], lambda: ran.append("other"), outside="skip")
    with pytest.raises(RuntimeError, match="poisoned"):
        _pass(body, poison=True)
    assert ran == [], "the engine drops its callbacks when a node raises"
    assert set(ops._END_MARKS) == {A, others[0]} and not ops.queued_at_end_of_backward(A)
    _pass(body)
    assert ran == ["a", "other"] and stale == [False, True]
    assert set(ops._END_MARKS) == {others[0]}
    # twice in a row
    with pytest.raises(RuntimeError, match="poisoned"):
        _pass(body, poison=True)
    with pytest.raises(RuntimeError, match="poisoned"):
        _pass(body, poison=True)
    assert set(ops._END_MARKS) == {A, others[0], others[2], others[3]}
    _pass(body)
    assert ran == ["a", "other"] * 2 and stale == [False, True, False, True, True]
    del others[:]
    gc.collect()                                    # the failed passes' marks go with their keys


def test_outside_a_pass():
    ran = []
    assert ops._graph_task() < 0
    ops.at_end_of_backward(A, lambda: ran.append("run"), outside="run")
    assert ran == ["run"]
    ops.at_end_of_backward(A, lambda: ran.append("skip"), outside="skip")
    assert ran == ["run"] and not ops.queued_at_end_of_backward(A)
    with pytest.raises(ValueError):
        ops.at_end_of_backward(A, lambda: None, outside="later")


def test_a_reentrant_pass_is_a_pass_of_its_own():
    ran, tasks = [], []

    def inner():
        tasks.append(ops._graph_task())
        ops.at_end_of_backward(A, lambda: ran.append("inner"), outside="skip")

    def outer():
        tasks.append(ops._graph_task())
        ops.at_end_of_backward(A, lambda: ran.append("outer"), outside="skip")
        with torch.enable_grad():
            _pass(inner)
        assert ran == ["inner"], "the inner pass's callback runs when the inner pass ends"
    _pass(outer)
    assert ran == ["inner", "outer"]
    assert len(tasks) == 2 and tasks[0] >= 0 and tasks[1] >= 0 and tasks[0] != tasks[1]
