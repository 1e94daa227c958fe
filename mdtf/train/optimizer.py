"""Optimizers (TF1 ``tf.train.*Optimizer`` API) on fused flat-buffer kernels.

Reference: ``@optimizer(optimizer=tf.train.AdamOptimizer(0.001))``
(``distribute.py:26``), the default Adam(1e-3) (``distribute.py:112``) and
``SyncReplicasOptimizer`` (``distribute_train.py:146-160``).

``compute_gradients`` / ``apply_gradients`` / ``minimize`` return *handles*
(see :mod:`mdtf.train.step`): the work runs when a session runs the returned
train op.  Updates are applied by one fused HIP launch per parameter group
(:mod:`mdtf.ops.optim`).  Optimizer slots keep TF's checkpoint names
(``<var>/Momentum``, ``<var>/Adam``, ``<var>/Adam_1``, ``beta1_power``,
``beta2_power``; LAMB: ``<var>/adam_m``, ``<var>/adam_v``).
"""
import torch
from ..ops import optim as K
from . import step as step_mod


def _lr_value(lr, global_step):
    if callable(lr):
        return float(lr(global_step))
    if hasattr(lr, "learning_rate"):        # mdtf.utils.learning_rate.LearningRate
        return float(lr.learning_rate)
    return float(lr)


def _clipnorm(value):
    if value is None:
        return None
    value = float(value)
    if value < 0 or value != value:
        raise ValueError("global_clipnorm must be a non-negative number, got %r" % (value,))
    return value or None


class Optimizer(object):
    slot_names = ()
    layerwise = False       # per-layer trust ratios (LAMB, LARS): update_all needs every target's reduced gradient

    def __init__(self, learning_rate, use_locking=False, name="Optimizer", weight_decay=0.0, global_clipnorm=None):
        self._lr = learning_rate
        self._name = name
        self.use_locking = use_locking
        self.weight_decay = float(weight_decay)
        # clip the averaged gradient by its global norm (tf.clip_by_global_norm, mdtf.train.clip_by_global_norm)
        # in every train op of this optimizer: for minimize() / the annotation-configured run loop / an
        # Estimator model_fn, which never expose the gradients.  None or 0: off.
        self.global_clipnorm = _clipnorm(global_clipnorm)
        self.last_global_norm = None    # [norm, coef] tensor of the last clipped step (set by the train op)

    def get_name(self):
        return self._name

    def learning_rate(self, global_step=0):
        return _lr_value(self._lr, global_step)

    # -- TF graph-building API (deferred) -------------------------------
    def compute_gradients(self, loss, var_list=None):
        return step_mod.compute_gradients(loss, var_list)

    def apply_gradients(self, grads_and_vars, global_step=None, name=None):
        return step_mod.TrainOp(self, grads_and_vars, global_step)

    def minimize(self, loss, global_step=None, var_list=None, name=None):
        if isinstance(loss, torch.Tensor):
            # inside an Estimator model_fn (re-run eagerly every step): the estimator
            # turns this request into ONE TrainOp over the recorded program's loss
            from ..estimator.estimator import current_capture
            cap = current_capture()
            if cap is None:
                raise TypeError("minimize() of a concrete tensor is only valid inside an Estimator model_fn; "
                                "use the loss handle returned by Tower.process()")
            return cap.record(self, global_step, var_list)
        return self.apply_gradients(self.compute_gradients(loss, var_list), global_step, name)

    # -- fused update over one UpdateTarget ------------------------------
    def update(self, target, lr, grad_scale, step, dyn=None):
        """One fused launch over ``target``.  ``dyn``: optional device tensor
        ``[lr, lr_t, grad_scale]`` overriding the scalars (hipGraph replay)."""
        raise NotImplementedError

    def update_all(self, targets, lr, grad_scale, step, dyn=None, reducer=None):
        """The update of every target of one step.  Layer-wise optimizers override it: their norms span targets'
        pieces (and, sharded, replicas: ``reducer`` sums them)."""
        for target in targets:
            self.update(target, lr, grad_scale, step, dyn=dyn)

    def step_size(self, lr, step):
        """The per-step ``lr_t`` the kernel applies (Adam folds its bias correction in)."""
        return lr

    def update_multi(self, target, grads, steps, grad_scale=1.0):
        """Apply ``grads`` (<= 8, in order) to ``target`` as consecutive updates at global ``steps``, in ONE
        fused pass (async parameter server).  Default: one ``update`` per gradient."""
        for g, st in zip(grads, steps):
            target.grad.copy_(g)
            self.update(target, self.learning_rate(st), grad_scale, st)

    def _wd(self, target):
        return self.weight_decay if target.decay else 0.0

    def slot_checkpoint_names(self):
        """(state name, TF slot suffix) pairs."""
        return []

    def extra_checkpoint_scalars(self, step):
        return {}


class GradientDescentOptimizer(Optimizer):
    def __init__(self, learning_rate, use_locking=False, name="GradientDescent", weight_decay=0.0,
                 global_clipnorm=None):
        super(GradientDescentOptimizer, self).__init__(learning_rate, use_locking, name, weight_decay,
                                                       global_clipnorm)

    def update(self, target, lr, grad_scale, step, dyn=None):
        K.sgd_(target.master, target.grad, target.shadow, lr, grad_scale, self._wd(target), dyn=dyn)

    def update_multi(self, target, grads, steps, grad_scale=1.0):
        lrs = [self.learning_rate(s) for s in steps]
        K.apply_multi_("sgd", target.master, grads, None, None, target.shadow, lrs, lrs, grad_scale=grad_scale,
                       weight_decay=self._wd(target))


class MomentumOptimizer(Optimizer):
    def __init__(self, learning_rate, momentum=0.9, use_locking=False, name="Momentum", use_nesterov=False,
                 weight_decay=0.0, global_clipnorm=None):
        super(MomentumOptimizer, self).__init__(learning_rate, use_locking, name, weight_decay, global_clipnorm)
        self.momentum = float(momentum)
        self.use_nesterov = use_nesterov

    def update(self, target, lr, grad_scale, step, dyn=None):
        K.momentum_(target.master, target.grad, target.state("momentum"), target.shadow, lr, self.momentum,
                    grad_scale, self._wd(target), self.use_nesterov, dyn=dyn)

    def update_multi(self, target, grads, steps, grad_scale=1.0):
        lrs = [self.learning_rate(s) for s in steps]
        K.apply_multi_("momentum", target.master, grads, target.state("momentum"), None, target.shadow, lrs, lrs,
                       momentum=self.momentum, grad_scale=grad_scale, weight_decay=self._wd(target),
                       flag=self.use_nesterov)

    def slot_checkpoint_names(self):
        return [("momentum", "Momentum")]


class AdamOptimizer(Optimizer):
    def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8, use_locking=False, name="Adam",
                 weight_decay=0.0, decoupled_weight_decay=False, bias_correction=True, global_clipnorm=None):
        super(AdamOptimizer, self).__init__(learning_rate, use_locking, name, weight_decay, global_clipnorm)
        self.beta1, self.beta2, self.epsilon = float(beta1), float(beta2), float(epsilon)
        self.decoupled = decoupled_weight_decay
        self.bias_correction = bias_correction

    def update(self, target, lr, grad_scale, step, dyn=None):
        K.adam_(target.master, target.grad, target.state("m"), target.state("v"), target.shadow, lr,
                self.beta1, self.beta2, self.epsilon, step + 1, grad_scale, self._wd(target), self.decoupled,
                self.bias_correction, dyn=dyn)

    def step_size(self, lr, step):
        return K.adam_lr_t(lr, self.beta1, self.beta2, step + 1, self.bias_correction)

    def update_multi(self, target, grads, steps, grad_scale=1.0):
        lrs = [self.learning_rate(s) for s in steps]
        lrts = [self.step_size(lr, s) for lr, s in zip(lrs, steps)]
        K.apply_multi_("adam", target.master, grads, target.state("m"), target.state("v"), target.shadow, lrs, lrts,
                       beta1=self.beta1, beta2=self.beta2, epsilon=self.epsilon, grad_scale=grad_scale,
                       weight_decay=self._wd(target), flag=self.decoupled)

    def slot_checkpoint_names(self):
        return [("m", "Adam"), ("v", "Adam_1")]

    def extra_checkpoint_scalars(self, step):
        return {"beta1_power": self.beta1 ** (step + 1), "beta2_power": self.beta2 ** (step + 1)}


class AdamWeightDecayOptimizer(AdamOptimizer):
    """BERT's optimizer: Adam without bias correction + decoupled weight decay.  BERT's recipe around it:
    ``learning_rate=mdtf.train.polynomial_decay(...)`` (linear warm-up + decay) and ``global_clipnorm=1.0``
    (``tf.clip_by_global_norm(grads, 1.0)``)."""

    def __init__(self, learning_rate, weight_decay_rate=0.01, beta_1=0.9, beta_2=0.999, epsilon=1e-6,
                 name="AdamWeightDecayOptimizer", global_clipnorm=None):
        super(AdamWeightDecayOptimizer, self).__init__(learning_rate, beta_1, beta_2, epsilon, name=name,
                                                       weight_decay=weight_decay_rate,
                                                       decoupled_weight_decay=True, bias_correction=False,
                                                       global_clipnorm=global_clipnorm)


class _LayerwiseOptimizer(Optimizer):
    """LAMB / LARS: ``update_all`` is one norm (or moments) launch per target, ONE ``layer_finalize`` launch over
    every layer of every target (one block per layer; sharded replicas all-reduce the fp64 sums between its two
    halves, captured like the bucket collectives) and one apply launch per target (:mod:`mdtf.ops.layerwise`).
    "Layers" are variables; the ratio applies to those with ``apply_weight_decay`` (rank > 1), the others take the
    plain step.  ``last_ratios``: the device tensor of the last step's per-layer ratios (layer order:
    ``last_layer_names``)."""
    layerwise = True

    def __init__(self, *args, **kwargs):
        super(_LayerwiseOptimizer, self).__init__(*args, **kwargs)
        self.last_ratios = None
        self.last_layer_names = None

    def update(self, target, lr, grad_scale, step, dyn=None):
        raise NotImplementedError("%s is layer-wise: a variable's norm spans update targets' pieces, use update_all"
                                  % type(self).__name__)

    def update_multi(self, target, grads, steps, grad_scale=1.0):
        raise NotImplementedError("%s has no multi-gradient update (ps_mode=async|sync_ps is not supported)"
                                  % type(self).__name__)

    def _norms(self, lmap, buf, ti, target, grad_scale, dyn):
        raise NotImplementedError

    def _finalize(self, lmap, buf, grad_scale, dyn, mode):
        raise NotImplementedError

    def _apply(self, lmap, buf, ti, target, lr, grad_scale, dyn):
        raise NotImplementedError

    def update_all(self, targets, lr, grad_scale, step, dyn=None, reducer=None):
        if not targets:
            return
        from ..ops import layerwise as LW
        lmap, buf = LW.state_for(targets, reducer)
        for ti, target in enumerate(targets):
            self._norms(lmap, buf, ti, target, grad_scale, dyn)
        if reducer is not None and reducer.mode == "sharded" and reducer.collective:
            self._finalize(lmap, buf, grad_scale, dyn, LW.REDUCE)
            reducer.all_reduce_sum(buf.sums)
            self._finalize(lmap, buf, grad_scale, dyn, LW.COEF)
        else:
            self._finalize(lmap, buf, grad_scale, dyn, LW.FULL)
        for ti, target in enumerate(targets):
            self._apply(lmap, buf, ti, target, lr, grad_scale, dyn)
        self.last_ratios, self.last_layer_names = buf.ratio, lmap.names


class LAMBOptimizer(_LayerwiseOptimizer):
    """LAMB as google-research's TF1 ``LAMBOptimizer`` (no bias correction; the code line of
    :class:`AdamWeightDecayOptimizer`)::

        m = b1 m + (1 - b1) g ;  v = b2 v + (1 - b2) g^2 ;  u = m / (sqrt(v) + eps) + wd w
        r = |w| / |u|  if |w| > 0 and |u| > 0 else 1 ;  w -= lr r u

    ``wd`` and ``r`` apply to variables with ``apply_weight_decay`` (rank > 1: not LayerNorm / bias); the others
    have ``wd = 0``, ``r = 1``.  ``g`` is the averaged gradient, clipped when ``global_clipnorm`` is set (BERT's
    recipe: ``global_clipnorm=1.0``).  Slots: ``<var>/adam_m``, ``<var>/adam_v``."""

    def __init__(self, learning_rate, weight_decay_rate=0.0, beta_1=0.9, beta_2=0.999, epsilon=1e-6,
                 name="LAMBOptimizer", global_clipnorm=None):
        super(LAMBOptimizer, self).__init__(learning_rate, False, name, weight_decay_rate, global_clipnorm)
        self.beta1, self.beta2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)

    def _norms(self, lmap, buf, ti, t, grad_scale, dyn):
        from ..ops import layerwise as LW
        LW.lamb_moments_(lmap, buf, ti, t.master, t.grad, t.state("m"), t.state("v"), self.beta1, self.beta2,
                         self.epsilon, grad_scale, self.weight_decay, dyn=dyn)

    def _finalize(self, lmap, buf, grad_scale, dyn, mode):
        from ..ops import layerwise as LW
        LW.layer_finalize_(lmap, buf, LW.LAMB, grad_scale=grad_scale, dyn=dyn, mode=mode)

    def _apply(self, lmap, buf, ti, t, lr, grad_scale, dyn):
        from ..ops import layerwise as LW
        LW.lamb_apply_(lmap, buf, ti, t.master, t.state("m"), t.state("v"), t.shadow, lr, self.epsilon,
                       self.weight_decay, dyn=dyn)

    def slot_checkpoint_names(self):
        return [("m", "adam_m"), ("v", "adam_v")]


class LARSOptimizer(_LayerwiseOptimizer):
    """LARS as ``tf.contrib.opt.LARSOptimizer``::

        decay variables:  t = eeta |w| / (|g| + wd |w| + eps)  if |w| > 0 and |g| > 0 else 1
                          s = lr t (g + wd w)
        other variables:  s = lr g
        acc = momentum acc + s ;  w -= acc          (nesterov: w -= s + momentum acc)

    "Decay variables" are those with ``apply_weight_decay`` (rank > 1), the set LARS's skip list leaves.  ``g``
    is the averaged (and, with ``global_clipnorm``, clipped) gradient.  Slot: ``<var>/Momentum``."""

    def __init__(self, learning_rate, momentum=0.9, weight_decay=1e-4, eeta=1e-3, epsilon=0.0, use_nesterov=False,
                 name="LARSOptimizer", global_clipnorm=None):
        super(LARSOptimizer, self).__init__(learning_rate, False, name, weight_decay, global_clipnorm)
        self.momentum, self.eeta, self.epsilon = float(momentum), float(eeta), float(epsilon)
        self.use_nesterov = use_nesterov

    def _norms(self, lmap, buf, ti, t, grad_scale, dyn):
        from ..ops import layerwise as LW
        LW.lars_norms_(lmap, buf, ti, t.master, t.grad)

    def _finalize(self, lmap, buf, grad_scale, dyn, mode):
        from ..ops import layerwise as LW
        LW.layer_finalize_(lmap, buf, LW.LARS, self.eeta, self.weight_decay, self.epsilon, grad_scale, dyn=dyn,
                           mode=mode)

    def _apply(self, lmap, buf, ti, t, lr, grad_scale, dyn):
        from ..ops import layerwise as LW
        LW.lars_apply_(lmap, buf, ti, t.master, t.grad, t.state("momentum"), t.shadow, lr, self.momentum, grad_scale,
                       self.weight_decay, self.use_nesterov, dyn=dyn)

    def slot_checkpoint_names(self):
        return [("momentum", "Momentum")]


class SyncReplicasOptimizer(Optimizer):
    """Synchronous data-parallel wrapper (``tf.train.SyncReplicasOptimizer``).

    ``replicas_to_aggregate`` of ``total_num_replicas`` gradients are averaged
    per step (backup workers when smaller).  ``mode='allreduce'`` reduces with
    overlapped bucketed all-reduce; ``mode='sharded'`` makes every rank the
    parameter server of 1/N of each bucket (reduce-scatter + local fused update
    + all-gather) — the MI355X-native form of PS variable sharding.
    ``bucket_bytes`` (default ``MDTF_BUCKET_MB`` or 32 MiB of fp32 gradients) sets the
    collective granularity; ``comm_dtype='bf16'`` halves the bytes on the wire.
    """

    def __init__(self, opt, replicas_to_aggregate=None, total_num_replicas=None, variable_averages=None,
                 variables_to_average=None, use_locking=False, name="sync_replicas", mode="allreduce",
                 bucket_bytes=None, overlap=True, hip_graph=None, comm_dtype=None, global_clipnorm=None):
        super(SyncReplicasOptimizer, self).__init__(opt._lr, use_locking, name, opt.weight_decay)
        self._opt = opt
        if global_clipnorm is not None:
            self.global_clipnorm = global_clipnorm      # held by the wrapped optimizer (property below)
        self.replicas_to_aggregate = replicas_to_aggregate
        self.total_num_replicas = total_num_replicas
        self.mode = mode
        self.bucket_bytes = bucket_bytes
        self.overlap = overlap
        self.hip_graph = hip_graph   # None: MDTF_HIP_GRAPH / --hip_graph decide (mdtf.train.graph)
        # gradient wire dtype: None -> MDTF_COMM_DTYPE (fp32 default) | "bf16" (mdtf.parallel.reducer)
        self.comm_dtype = comm_dtype

    @property
    def global_clipnorm(self):
        opt = self.__dict__.get("_opt")
        return opt.global_clipnorm if opt is not None else None

    @global_clipnorm.setter
    def global_clipnorm(self, value):
        opt = self.__dict__.get("_opt")
        if opt is not None:
            opt.global_clipnorm = _clipnorm(value)

    def learning_rate(self, global_step=0):
        return self._opt.learning_rate(global_step)

    def update(self, target, lr, grad_scale, step, dyn=None):
        self._opt.update(target, lr, grad_scale, step, dyn=dyn)

    def update_multi(self, target, grads, steps, grad_scale=1.0):
        self._opt.update_multi(target, grads, steps, grad_scale)

    @property
    def layerwise(self):
        return self._opt.layerwise

    def update_all(self, targets, lr, grad_scale, step, dyn=None, reducer=None):
        self._opt.update_all(targets, lr, grad_scale, step, dyn=dyn, reducer=reducer)

    def step_size(self, lr, step):
        return self._opt.step_size(lr, step)

    def slot_checkpoint_names(self):
        return self._opt.slot_checkpoint_names()

    def extra_checkpoint_scalars(self, step):
        return self._opt.extra_checkpoint_scalars(step)

    def apply_gradients(self, grads_and_vars, global_step=None, name=None):
        op = step_mod.TrainOp(self, grads_and_vars, global_step, sync=True)
        return op

    def make_session_run_hook(self, is_chief, num_tokens=-1):
        from .hooks import SyncReplicasHook
        return SyncReplicasHook(self, is_chief)

    def get_init_tokens_op(self, num_tokens=-1):
        return None

    def get_chief_queue_runner(self):
        return None


def polynomial_decay(learning_rate, decay_steps, end_learning_rate=0.0, power=1.0, warmup_steps=0):
    """``tf.train.polynomial_decay`` with BERT's linear warm-up (``optimization.py``), as a callable of
    ``global_step`` to pass as an optimizer's ``learning_rate``::

        step <  warmup_steps:  learning_rate * step / warmup_steps
        else:                  (learning_rate - end) * (1 - min(step, decay_steps) / decay_steps) ** power + end

    The per-step value reaches a replayed hipGraph through the device hyper-parameter buffer (no re-capture)."""
    lr0, end, power = float(learning_rate), float(end_learning_rate), float(power)
    decay_steps, warmup_steps = int(decay_steps), int(warmup_steps)
    if decay_steps <= 0:
        raise ValueError("decay_steps must be positive, got %r" % (decay_steps,))

    def schedule(global_step):
        step = int(global_step)
        if step < warmup_steps:
            return lr0 * step / warmup_steps
        frac = 1.0 - min(step, decay_steps) / float(decay_steps)
        return (lr0 - end) * frac ** power + end
    return schedule


# aliases with TF spellings
Adam = AdamOptimizer
Momentum = MomentumOptimizer
GradientDescent = GradientDescentOptimizer
