"""``tf.train.ExponentialMovingAverage`` of the weights, updated on the device inside the training step.

    ema = mdtf.train.ExponentialMovingAverage(0.9999, num_updates=global_step)
    train_op = ema.apply(train_op=train_op)        # the same handle: fetching it runs the step, then the average

TF keeps one shadow variable per variable and updates it with ``shadow -= (1 - decay) * (shadow - var)`` under
``tf.control_dependencies([train_op])``.  Here the averages live beside the flat fp32 masters as per-target state
(``target.state("ema")``: full buffers in all-reduce mode, each rank's own shard in sharded mode, like ``m``, ``v``
and ``Momentum``) and one launch per update target (:mod:`mdtf.ops.ema`) updates them at the end of the step, after
the optimizer's updates.  No collective is added; sharded mode keeps its in-backward update / all-gather overlap.

``num_updates`` (None, an int or the global step) gives TF's ``min(decay, (1 + n) / (10 + n))``; ``n`` is read
AFTER the step's increment, as under ``tf.control_dependencies([train_op])``: the first update of a fresh run uses
``n = 1``.  ``1 - decay`` is formed on the host in double and rounded to fp32 once; a replayed hipGraph reads it
from a 1-float device buffer this object owns, refreshed between replays only when it changed.

The average of a variable starts as the variable's value before the first step (TF's shadow initialiser).
Checkpoints carry it as ``<var>/ExponentialMovingAverage`` (:mod:`mdtf.train.saver`).

Not supported: ``zero_debias=True``, a strict subset of the train op's variables (the averages cover the whole
flat space), ``ps_mode=async|sync_ps`` and the Estimator front end.
"""
import contextlib

import torch

from ..ops import ema as K
from . import step as step_mod
from . import variables as V


class ExponentialMovingAverage(object):
    def __init__(self, decay, num_updates=None, zero_debias=False, name="ExponentialMovingAverage"):
        if zero_debias:
            raise NotImplementedError("ExponentialMovingAverage(zero_debias=True) is not supported")
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError("decay must be in [0, 1], got %r" % (decay,))
        if num_updates is not None and not isinstance(num_updates, V.GlobalStep):
            num_updates = int(num_updates)
        self.decay = decay
        self.num_updates = num_updates
        self.name = name
        self.op = None                  # the TrainOp this average is attached to (apply)
        self.initialized = False        # the state buffers hold the averages (first eager step / restore)
        self.omd_buf = None             # 1-float device buffer a captured step reads 1 - decay from
        self._omd_dev_val = None        # the value it holds

    # -- graph-building API ------------------------------------------------
    def apply(self, var_list=None, train_op=None):
        """Attach the average to ``train_op`` (from ``apply_gradients``, ``minimize`` or a
        ``SyncReplicasOptimizer``; None: the one registered train op) and return that handle."""
        if train_op is None:
            ops = step_mod.train_ops()
            if len(ops) != 1:
                raise ValueError("ExponentialMovingAverage.apply(train_op=None) needs exactly one registered train "
                                 "op, found %d: pass train_op=" % len(ops))
            train_op = ops[0]
        if not isinstance(train_op, step_mod.TrainOp):
            raise TypeError("apply expects the train op returned by apply_gradients / minimize, got %r" % (train_op,))
        if train_op.ema is not None:
            raise ValueError("this train op already has a moving average attached")
        if self.op is not None:
            raise ValueError("this ExponentialMovingAverage is already attached to a train op")
        if var_list is not None:
            store = V.get_store()
            names = set((store.vars[v] if isinstance(v, str) else v).name for v in var_list)
            have = set(v.name for v in train_op.variables)
            if names - have:
                raise ValueError("var_list holds variables the train op does not update: %s" % sorted(names - have)[:8])
            if names != have:
                raise NotImplementedError("ExponentialMovingAverage over a strict subset of the train op's variables "
                                          "is not supported: the averages cover every variable of the flat space")
        train_op.release_graph()        # a step captured without the average does not update it
        train_op.ema = self
        self.op = train_op
        return train_op

    def average_name(self, var):
        return "%s/%s" % (var.name if not isinstance(var, str) else var, self.name)

    def variables_to_restore(self):
        """``{checkpoint name: variable}`` for ``Saver``: trainable variables under their average's name, every
        other global variable (BN moving statistics ...) and ``global_step`` under their own."""
        out = {}
        for v in V.get_store().global_variables():
            out[self.average_name(v) if v.trainable else v.name] = v
        gs = V.get_global_step()
        if gs is not None:
            out[gs.name] = gs
        return out

    # -- decay ---------------------------------------------------------------
    def decay_at(self, step):
        """The decay of the update that follows the step run at global step ``step`` (its value before the
        increment)."""
        n = self.num_updates
        if n is None:
            return self.decay
        if isinstance(n, V.GlobalStep):
            # after the increment; another counter than the train op's own is read as it stands
            n = step + 1 if (self.op is not None and n is self.op.global_step) else n.value()
        return min(self.decay, (1.0 + n) / (10.0 + n))

    def omd_at(self, step):
        return K.one_minus_decay(self.decay_at(step))

    # -- state ---------------------------------------------------------------
    def _reducer(self):
        if self.op is None:
            raise RuntimeError("this ExponentialMovingAverage is not attached to a train op: call apply() first")
        if self.op.space is None:
            self.op.finalize()
        return self.op.reducer

    def _alloc_guard(self):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("moving-average buffers must be allocated by an eager step before capture")

    def ensure_initialized(self):
        """Allocate the state (``full/ema`` or ``shard/ema`` of every group) and fill it from the masters: the
        first eager step calls this before its optimizer update."""
        if self.initialized:
            return
        self._alloc_guard()
        with torch.no_grad():
            for t in self._reducer().all_targets():
                t.state("ema").copy_(t.master)
        self.initialized = True

    def device_omd(self, step):
        """The 1-float device buffer holding ``1 - decay`` of ``step``, copied only when the value changed
        (between hipGraph replays; the captured launch reads the buffer)."""
        val = self.omd_at(step)
        if self.omd_buf is None:
            self._alloc_guard()
            self.omd_buf = torch.zeros(1, dtype=torch.float32, device=self._reducer().space.groups[0].device)
            self._omd_dev_val = None
        if val != self._omd_dev_val:
            host = torch.tensor([val], dtype=torch.float32)
            if self.omd_buf.is_cuda:
                host = host.pin_memory()
            self.omd_buf.copy_(host, non_blocking=True)
            self._omd_dev_val = val
        return self.omd_buf

    def update(self, step, captured=False):
        """The update of every target, at the end of ``TrainOp._run_step``.  ``captured``: read the decay from the
        device buffer (``StepGraph`` refreshes it before each replay); eager steps pass the scalar."""
        omd = self.omd_at(step)
        dev = self.omd_buf if captured else None
        if captured and dev is None:
            raise RuntimeError("moving-average decay buffer must be allocated before capture")
        with torch.no_grad():
            for t in self._reducer().all_targets():
                K.ema_update_(t.state("ema"), t.master, omd, omd_dev=dev)

    def load_full(self, fulls):
        """Restore: one full-size fp32 buffer per group (each rank keeps its shard in sharded mode)."""
        self._alloc_guard()
        self._reducer().scatter_full_state("ema", fulls)
        self.initialized = True

    def full_state(self):
        """One full-size buffer per group (sharded: gathered, collective)."""
        self.ensure_initialized()
        return self._reducer().gather_full_state(None, "ema")

    # -- accessors -----------------------------------------------------------
    def average(self, var):
        """The average of ``var``: an fp32 tensor of ``var.shape`` (a copy).  Sharded mode gathers it: every
        replica must call."""
        if isinstance(var, str):
            var = V.get_store().vars[var]
        red = self._reducer()
        fulls = self.full_state()
        for g, full in zip(red.space.groups, fulls):
            if var.flat_group is g:
                o = var.flat_offset
                return full[o:o + var.numel()].view(var.shape).clone()
        raise ValueError("%s is not a variable of the train op this average is attached to" % var.name)

    @contextlib.contextmanager
    def average_weights(self):
        """Evaluate on the averaged weights inside a training job: masters and averages are exchanged in place
        (data moves, pointers stay: the buffers are baked into a captured graph), the compute shadows and, in
        sharded mode, every rank's full masters refreshed; exchanged back on exit.  Collective in sharded mode."""
        red = self._reducer()
        self.ensure_initialized()
        self._exchange(red)
        try:
            yield self
        finally:
            self._exchange(red)

    def _exchange(self, red):
        with torch.no_grad():
            for t in red.all_targets():
                e = t.state("ema")
                tmp = t.master.clone()
                t.master.copy_(e)
                e.copy_(tmp)
            # every rank's full masters (sharded: gathered, fp32 groups too) and compute shadows follow
            red.gather_full_master(include_fp32=True)
            red.space.refresh_shadows()
