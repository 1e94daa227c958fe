"""``Eval`` operator — a real evaluation loop (the reference's is a stub,
``distribute_eval.py:13-23``).

Builds the model forward from ``data_loader.load_eval_batch()`` under the same
variable names, restores the latest checkpoint from ``model_dir`` (waiting for
one up to ``checkpoint_wait_secs``), runs ``eval_steps`` batches in inference
mode (BN uses moving statistics) and reports mean loss and — when the logits
are class scores and the ground truth integer labels — top-1 accuracy and
``top_<k>_accuracy`` (``--eval_top_k``, default 5, for more than k classes),
plus whatever the ``Loss.metrics`` hook returns, under its names.  Any other
``logits`` (a tuple, as BERT's) get the loss and the hook's metrics.  All of
them are ``mdtf.metrics`` accumulated on the device and read once after the
loop.  Eval tasks of a multi-replica job shard the batches and all-reduce the
sums; every replica must report the same metric names.
"""
import time

import torch

from ..config.flags import FLAGS
from ..data.loaders import InputOptions
from ..train import saver as SV
from ..train import step as S
from ..train import variables as V
from ..utils import log as logger
from .tower import Tower


def pack_sums(steps, loss_acc, correct_acc, extras, device):
    """The fp64 vector a multi-replica Eval all-reduces, built on ``device`` without a host read:
    ``[loss total, correct, count, steps]`` followed by ``{total, count}`` of every accumulator in ``extras``."""
    parts = [loss_acc.tensor[:1], correct_acc.tensor, torch.tensor([float(steps)], dtype=torch.float64)]
    parts += [a.tensor for a in extras]
    return torch.cat([p.to(device) for p in parts])


def unpack_sums(t, names):
    """``(loss total, correct, count, steps, {name: (total, count)})`` from the vector of :func:`pack_sums`; the
    one host read of an evaluation."""
    v = t.tolist()
    if len(v) != 4 + 2 * len(names):
        raise ValueError("expected %d sums for %r, got %d" % (4 + 2 * len(names), names, len(v)))
    return v[0], v[1], v[2], v[3], {n: (v[4 + 2 * i], v[5 + 2 * i]) for i, n in enumerate(names)}


class Eval(object):
    def __init__(self, data_loader=None, input_mode=None):
        self.data_loader = data_loader
        self.input_mode = input_mode

    def eval(self, pre_eval_fn=None, post_eval_fn=None, pre_process_fn=None, post_process_fn=None, *args, **kwargs):
        from .train import configure_store_for
        server = getattr(self, "server", None)
        if server is not None and self.job_name == "ps":
            return None
        configure_store_for(server)
        pre = pre_eval_fn(args, kwargs) if pre_eval_fn is not None else None
        if self.input_mode == InputOptions.PLACEHOLDER:
            raw, gt = self.data_loader.load_eval_batch()
        else:
            raw, gt = self.data_loader.load_eval_batch()
        tower = Tower(self.net, "tower_0/", [], raw, gt, self.loss, None, pre_process_fn=pre_process_fn,
                      batch_size=self.batch_size)
        with S.training_mode(False):
            loss_h, logits_h = tower.tower_loss(post_process_fn, pre)
        V.get_store().frozen = True           # variables exist now: later forwards reuse them
        V.get_or_create_global_step()
        ckpt = self._wait_for_checkpoint()
        if ckpt is not None:
            self._restore(ckpt)
            logger.info("Eval: restored %s (global_step %d)" % (ckpt, V.get_global_step().value()))
        else:
            logger.warn("Eval: no checkpoint in %r; evaluating the initial weights" % (self.model_dir,))
        steps = int(getattr(self, "eval_steps", 0) or max(self.sample_number // max(self.batch_size, 1), 1))
        from .. import metrics as M
        top_k = getattr(self, "eval_top_k", None)                   # an attribute of 0 switches a set flag off
        top_k = int((FLAGS.eval_top_k if top_k is None else top_k) or 0)
        loss_metrics = getattr(self.loss, "metrics", None)
        # streaming state on the device: nothing is read by the host before the loop ends
        loss_acc, correct_acc, extra = M.Accumulator(), M.Accumulator(), {}
        sample_queue = None
        if self.input_mode == InputOptions.PLACEHOLDER:
            sample_queue = self.data_loader.load_queue_for_placeholder(self.data_dir)
        for _ in range(steps):
            feed = None
            if sample_queue is not None:
                rb, gb = self.data_loader.load_placeholder_data(sample_queue)
                feed = {raw: rb, gt: gb}
            ctx = S.RunContext(feed)
            try:
                out = tower.program.forward(ctx, grad=False)
            except StopIteration:
                break
            logits = out["logits"]
            labels = tower._ground_truth_value
            with torch.no_grad():
                M.mean(out["loss"].detach().float().reshape(1), accumulator=loss_acc)
                if (isinstance(logits, torch.Tensor) and logits.dim() == 2 and isinstance(labels, torch.Tensor)
                        and not labels.is_floating_point() and labels.dim() == 1):
                    M.accuracy(labels, logits.argmax(-1), accumulator=correct_acc)
                    if 0 < top_k < logits.shape[1]:
                        M.top_k_accuracy(labels, logits, top_k,
                                         accumulator=extra.setdefault("top_%d_accuracy" % top_k, M.Accumulator()))
                hooked = loss_metrics(logits, labels) if loss_metrics is not None else None
                for name, mv in (hooked or {}).items():
                    extra.setdefault(name, M.Accumulator()).update(mv)
        names = sorted(extra)
        dev = V.get_store().device if V.get_store().device.type == "cuda" else torch.device("cpu")
        t = pack_sums(steps, loss_acc, correct_acc, [extra[n] for n in names], dev)
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and server is not None and server.worker_group is not None:
            dist.all_reduce(t, group=server.worker_group)           # every replica reports the same names
        total_loss, correct, count, steps, sums = unpack_sums(t, names)
        self.metrics = {"loss": total_loss / max(steps, 1),
                        "accuracy": (correct / count) if count else None,
                        "global_step": V.get_global_step().value(), "steps": int(steps)}
        for n in names:
            self.metrics[n] = (sums[n][0] / sums[n][1]) if sums[n][1] else 0.0
        logger.info("Eval: %s" % self.metrics)
        if server is not None:
            server.signal_done()
        if post_eval_fn is not None:
            post_eval_fn(args, kwargs)
        return self.metrics

    def _restore(self, ckpt):
        """--moving_average_decay (or the ``moving_average_decay`` attribute): restore every trainable variable
        from its ``<var>/ExponentialMovingAverage`` entry, i.e. evaluate the averaged weights; a checkpoint
        written without averages is evaluated on its raw weights, with a warning."""
        decay = getattr(self, "moving_average_decay", None)         # an attribute of 0 switches a set flag off
        decay = float((FLAGS.moving_average_decay if decay is None else decay) or 0.0)
        self.evaluated_averages = False
        if decay > 0:
            from ..ckpt.tensor_bundle import BundleReader
            from ..train.moving_averages import ExponentialMovingAverage
            ema = ExponentialMovingAverage(decay)
            reader = BundleReader(ckpt)
            wanted = [ema.average_name(v) for v in V.get_store().trainable_variables()]
            if wanted and all(k in reader for k in wanted):
                SV.Saver(ema.variables_to_restore()).restore(None, ckpt, reader=reader)
                self.evaluated_averages = True
                return
            logger.warn("Eval: %s holds no moving averages (%s/...): evaluating the raw weights" % (ckpt, ema.name))
        SV.Saver(save_optimizer_state=False).restore(None, ckpt)

    def _wait_for_checkpoint(self):
        md = getattr(self, "model_dir", None)
        wait = float(getattr(self, "checkpoint_wait_secs", 0))
        t0 = time.time()
        while True:
            ckpt = SV.latest_checkpoint(md) if md else None
            if ckpt or time.time() - t0 >= wait:
                return ckpt
            time.sleep(1.0)

    def run(self):
        return self.eval(pre_eval_fn=getattr(self, "pre_fn", None), post_eval_fn=getattr(self, "post_fn", None),
                         pre_process_fn=getattr(self, "pre_process_fn", None),
                         post_process_fn=getattr(self, "post_process_fn", None))
