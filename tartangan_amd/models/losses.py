"""models/losses.py of the reference, on the HIP kernels.

``gradient_penalty`` (R1, reference models/losses.py:17-30) is the function that
forces double backward through the discriminator.  The hinge losses
(losses.py:7-14) are assigned by the trainers (cnn.py:86-87) but never called; they are
here for API parity, composed from the twice-differentiable primitives (relu = LeakyReLU(0)).
"""
import torch

from .. import functional as TF


def _mean(x):
    return TF._RowSum.apply(x, x.dim(), 1.0 / x.numel())


def discriminator_hinge_loss(real, fake):
    """(mean relu(1 - real), mean relu(1 + fake))  (losses.py:7-10)"""
    ones_r, ones_f = torch.ones_like(real), torch.ones_like(fake)
    loss_real = _mean(TF.leaky_relu(TF.add(ones_r, TF.scale(real, -1.0)), 0.0))
    loss_fake = _mean(TF.leaky_relu(TF.add(ones_f, fake), 0.0))
    return loss_real, loss_fake


def generator_hinge_loss(fake):
    """-mean(fake)  (losses.py:13-14)"""
    return _mean(TF.scale(fake, -1.0))


def _graph_nodes(root, stop=()):
    """Nodes reachable from ``root`` without entering ``stop``."""
    seen, stack = set(), [root]
    while stack:
        node = stack.pop()
        if node is None or node in seen or node in stop:
            continue
        seen.add(node)
        stack.extend(fn for fn, _ in node.next_functions)
    return seen


def _order_second_order_nodes(first_order_root, grad_root):
    """Give the nodes that the ``create_graph`` pass just built a place in the engine's execution order that does not depend
    on the process's history.

    The autograd engine runs ready nodes by descending sequence number, and sequence numbers come from a per-thread
    counter.  The forward nodes are numbered by the calling thread; the nodes of a ``create_graph`` backward on a GPU are
    created -- and numbered -- by the engine's device thread, whose counter advances at another rate (measured: 145 per
    step against 125 on the 32-pixel CNN trainer).  Over the first steps of a process the new nodes' range climbs through
    the forward nodes' range, and the eager step's kernel order changed at every one of those steps (1 to 4 there) until the
    ranges had passed each other.  Where a double-backward node and a forward node that accumulate into the same ``.grad``
    swap places, the sums differ in the last place; a captured HIP graph meanwhile keeps the order of its capture.  Here
    the new nodes are renumbered to lie directly BELOW every forward node of this graph, in the order they were created:
    the order of the first step of a fresh process, at every step.

    The first graph of a process has no room below its forward nodes (they start near 0): those are shifted up first.  The
    nodes made around them by the caller -- the loss on ``preds`` before this call, ``sumsq`` / scale / add after it -- are
    not reachable from here and keep their numbers.  That changes nothing: ``sumsq`` / scale / add consume, directly or not,
    every node numbered here, and the loss on ``preds`` every forward node, so they run before those whatever their
    numbers; and the loss on ``preds``, the only one that can be ready beside the NEW nodes, was created after all forward
    nodes, which outnumber the new ones in these discriminators -- it stays above the new nodes with or without the shift.

    This rests on torch internals: the private ``Node._sequence_nr`` / ``_set_sequence_nr``, the engine's ready queue
    ordering by sequence number, and gradient accumulators being recognisable by the type name ``AccumulateGrad`` (they
    carry the maximal number and must keep it).  Verified on torch 2.10.  A torch that orders differently would not fail
    loudly: the symptom is last-place differences between graph replay and eager steps, which
    ``tests/test_step_transitions_gpu.py`` (bit equality) catches.  Without the setter the numbering is left as torch made
    it -- the earlier behaviour."""
    if not hasattr(grad_root, '_set_sequence_nr') or not hasattr(grad_root, '_sequence_nr'):
        return
    forward = _graph_nodes(first_order_root)
    new = sorted((n for n in _graph_nodes(grad_root, stop=forward) if type(n).__name__ != 'AccumulateGrad'),
                 key=lambda n: n._sequence_nr())
    numbered = [n for n in forward if type(n).__name__ != 'AccumulateGrad']
    if not new or not numbered:
        return
    base = min(n._sequence_nr() for n in numbered)
    if base < len(new):                          # (the first graph of a process: make room below)
        shift = len(new) - base
        for n in numbered:
            n._set_sequence_nr(n._sequence_nr() + shift)
        base += shift
    for k, n in enumerate(new):
        n._set_sequence_nr(base - len(new) + k)


def gradient_penalty(preds, data):
    """mean_b sum_chw (d sum(preds) / d data)^2, differentiable w.r.t. the D parameters."""
    batch_size = data.size(0)
    total = TF._RowSum.apply(preds, preds.dim(), 1.0)           # preds.sum()
    with TF.input_grads_only():                                 # d/d(data) only: no parameter gradients in this pass
        grad_dout = torch.autograd.grad(
            outputs=total, inputs=data, create_graph=True, retain_graph=True, only_inputs=True)[0]
    assert grad_dout.size() == data.size()
    if grad_dout.grad_fn is not None and total.grad_fn is not None:
        _order_second_order_nodes(total.grad_fn, grad_dout.grad_fn)
    return TF.sumsq(grad_dout, 1.0 / batch_size)
