"""Layer toolkit — the ``distribute_tools.py`` API on MI355X kernels.

Every function keeps the reference's name, arguments, variable names
(``weights``/``biases``/``weights_nonacti``/``biases_nonacti`` under the
``layer_name`` scope, SURVEY §9.5 — these become checkpoint tensor names) and
TF layouts (NHWC activations, HWIO filters).  Compute runs on the fused HIP
kernels of :mod:`mdtf.ops` (conv + bias + ReLU in one epilogue, BN statistics +
normalise + ReLU (+ residual) fused, ...).

Fixes: ``norm`` returns the LRN output (Q17); ``batch_norm`` is a
standard per-channel BN with affine parameters and moving statistics (Q18) —
``batch_norm(x, legacy=True)`` keeps the reference's batch-axis-only,
affine-free behaviour.
"""
import torch

from ..config.flags import FLAGS
from ..ops import nn as ops
from ..train import variables as V


def _dtype():
    return torch.float32  # masters are fp32; FLAGS.use_fp16 selects bf16 *compute* (see Train)


def _variable_on_cpu(name, shape, initializer):
    """Create/reuse a variable (``distribute_tools.py:24-38``).

    The name is historical: variables live in the HBM of the rank that owns
    them; the fp16 flag selects reduced-precision compute, not storage.
    """
    return V.get_variable(name, shape, dtype=_dtype(), initializer=initializer)


def _variable_with_weight_decay(name, shape, stddev, wd):
    """Truncated-normal variable; adds ``wd * l2_loss(var)`` to 'losses' (``:41-66``)."""
    var = _variable_on_cpu(name, shape, V.truncated_normal_initializer(stddev=stddev))
    if wd is not None and wd != 0.0:
        store = V.get_store()
        scope = V.get_variable_scope().name
        full = "%s/%s" % (scope, name) if scope else name
        V.add_to_collection("losses", ops.l2_loss(store.vars[full].read(store.compute_dtype)) * wd)
    return var


def _strides(stride):
    return stride


def conv(layer_name, x, in_channels, out_channels, kernel_size=(3, 3), stride=(1, 1, 1, 1)):
    """conv (SAME) + bias + ReLU in one fused kernel (``distribute_tools.py:69-79``)."""
    with V.variable_scope(layer_name):
        return _conv_body(x, in_channels, out_channels, kernel_size, stride)


def conv_eval(layer_name, x, in_channels, out_channels, kernel_size=(3, 3), stride=(1, 1, 1, 1)):
    """``conv`` with AUTO_REUSE (``:81-91``)."""
    with V.variable_scope(layer_name, reuse=V.AUTO_REUSE):
        return _conv_body(x, in_channels, out_channels, kernel_size, stride)


def _conv_body(x, in_channels, out_channels, kernel_size, stride):
    w = _variable_with_weight_decay('weights', [kernel_size[0], kernel_size[1], in_channels, out_channels],
                                    stddev=5e-2, wd=0.0)
    b = _variable_on_cpu('biases', [out_channels], V.constant_initializer(0.0))
    return ops.conv2d(x, w, _strides(stride), "SAME", bias=b, act="relu")


def conv_nonacti(layer_name, x, in_channels, out_channels, kernel_size=(3, 3), stride=(1, 1, 1, 1)):
    """conv + bias, no activation; Xavier init (``:93-105``)."""
    with V.variable_scope(layer_name):
        return _conv_nonacti_body(x, in_channels, out_channels, kernel_size, stride)


def conv_nonacti_eval(layer_name, x, in_channels, out_channels, kernel_size=(3, 3), stride=(1, 1, 1, 1)):
    with V.variable_scope(layer_name, reuse=V.AUTO_REUSE):
        return _conv_nonacti_body(x, in_channels, out_channels, kernel_size, stride)


def _conv_nonacti_body(x, in_channels, out_channels, kernel_size, stride):
    w = V.get_variable('weights_nonacti', [kernel_size[0], kernel_size[1], in_channels, out_channels],
                       initializer=V.xavier_initializer())
    b = V.get_variable('biases_nonacti', [out_channels], initializer=V.constant_initializer(0.0))
    return ops.conv2d(x, w, _strides(stride), "SAME", bias=b)


def depthwise_conv(layer_name, x, in_channels, kernel_size=(3, 3), stride=(1, 1, 1, 1), channel_multiplier=1):
    """Depthwise conv (SAME) + bias + ReLU; variables ``depthwise_weights`` and ``biases`` (slim's names)."""
    with V.variable_scope(layer_name):
        return _depthwise_body(x, in_channels, kernel_size, stride, channel_multiplier)


def depthwise_conv_eval(layer_name, x, in_channels, kernel_size=(3, 3), stride=(1, 1, 1, 1), channel_multiplier=1):
    """``depthwise_conv`` with AUTO_REUSE."""
    with V.variable_scope(layer_name, reuse=V.AUTO_REUSE):
        return _depthwise_body(x, in_channels, kernel_size, stride, channel_multiplier)


def _depthwise_weights(in_channels, kernel_size, channel_multiplier):
    return _variable_with_weight_decay('depthwise_weights',
                                       [kernel_size[0], kernel_size[1], in_channels, channel_multiplier],
                                       stddev=5e-2, wd=0.0)


def _depthwise_body(x, in_channels, kernel_size, stride, channel_multiplier):
    w = _depthwise_weights(in_channels, kernel_size, channel_multiplier)
    b = _variable_on_cpu('biases', [in_channels * channel_multiplier], V.constant_initializer(0.0))
    return ops.bias_add_relu(ops.depthwise_conv2d(x, w, _strides(stride), "SAME"), b)


def depthwise_conv_nonacti(layer_name, x, in_channels, kernel_size=(3, 3), stride=(1, 1, 1, 1),
                           channel_multiplier=1):
    """Depthwise conv (SAME), no bias, no activation: the form that precedes :func:`batch_norm`."""
    with V.variable_scope(layer_name):
        w = _depthwise_weights(in_channels, kernel_size, channel_multiplier)
        return ops.depthwise_conv2d(x, w, _strides(stride), "SAME")


def separable_conv(layer_name, x, in_channels, out_channels, kernel_size=(3, 3), stride=(1, 1, 1, 1),
                   channel_multiplier=1):
    """Depthwise conv (SAME) then a 1x1 conv + bias + ReLU (the ReLU after the pointwise conv only); variables
    ``depthwise_weights``, ``pointwise_weights`` and ``biases``."""
    with V.variable_scope(layer_name):
        dwf = _depthwise_weights(in_channels, kernel_size, channel_multiplier)
        pwf = _variable_with_weight_decay('pointwise_weights', [1, 1, in_channels * channel_multiplier, out_channels],
                                          stddev=5e-2, wd=0.0)
        b = _variable_on_cpu('biases', [out_channels], V.constant_initializer(0.0))
        return ops.bias_add_relu(ops.separable_conv2d(x, dwf, pwf, _strides(stride), "SAME"), b)


def acti_layer(x):
    """ReLU (``:123-128``)."""
    return ops.relu(x)


def deconv(layer_name, x, in_channels, out_channels, output_shape=(32, 224, 224, 64), kernel_size=(3, 3),
           stride=(1, 1, 1, 1)):
    """Transposed conv, no bias (``:131-143``).

    As in the reference the filter is created ``[kh, kw, in_channels, out_channels]``
    and interpreted with TF's transposed-conv layout ``[kh, kw, C_out_of_op, C_in_of_op]``.
    """
    with V.variable_scope(layer_name):
        return _deconv_body(x, in_channels, out_channels, output_shape, kernel_size, stride)


def deconv_eval(layer_name, x, in_channels, out_channels, output_shape=(32, 224, 224, 64), kernel_size=(3, 3),
                stride=(1, 1, 1, 1)):
    with V.variable_scope(layer_name, reuse=V.AUTO_REUSE):
        return _deconv_body(x, in_channels, out_channels, output_shape, kernel_size, stride)


def _deconv_body(x, in_channels, out_channels, output_shape, kernel_size, stride):
    w = V.get_variable('weights', [kernel_size[0], kernel_size[1], in_channels, out_channels],
                       initializer=V.xavier_initializer())
    return ops.conv2d_transpose(x, w, output_shape, _strides(stride), "SAME")


def pool(layer_name, x, kernel=(1, 2, 2, 1), stride=(1, 2, 2, 1), is_max_pool=True):
    """2x2/2 SAME max (default) or average pool (``:160-165``)."""
    if is_max_pool:
        return ops.max_pool(x, kernel, stride, "SAME", name=layer_name)
    return ops.avg_pool(x, kernel, stride, "SAME", name=layer_name)


def batch_norm(x, legacy=False, training=True, decay=0.9, epsilon=1e-3, relu=False, residual=None,
               name="batch_norm"):
    """Batch normalisation.

    ``legacy=True`` reproduces ``distribute_tools.py:168-180`` exactly
    (moments over axis 0 only, no offset/scale, no moving statistics).
    Otherwise: per-channel BN with ``gamma``/``beta`` and moving statistics,
    fused with optional residual add and ReLU.
    """
    if legacy:
        mean, var = ops.moments(x, [0])
        return ops.batch_normalization(x, mean, var, None, None, epsilon)
    c = x.shape[-1]
    with V.variable_scope(name, reuse=V.AUTO_REUSE if V.get_store().frozen else None):
        gamma = V.get_variable('gamma', [c], initializer=V.constant_initializer(1.0), keep_fp32=True)
        beta = V.get_variable('beta', [c], initializer=V.constant_initializer(0.0), keep_fp32=True)
        mm = V.get_variable('moving_mean', [c], initializer=V.constant_initializer(0.0), trainable=False)
        mv = V.get_variable('moving_variance', [c], initializer=V.constant_initializer(1.0), trainable=False)
    return ops.batch_norm(x, gamma, beta, mm, mv, training, decay, epsilon, relu, residual)


def group_norm(x, groups=32, epsilon=1e-6, relu=False, name="GroupNorm"):
    """``tf.contrib.layers.group_norm``: statistics per image over H, W and each of ``groups`` runs of adjacent
    channels, with ``<name>/gamma`` (ones) and ``<name>/beta`` (zeros), TF contrib's variable names.
    ``groups=C`` is instance normalization; ``groups=1`` is layer normalization over (H, W, C)."""
    c = x.shape[-1]
    with V.variable_scope(name, reuse=V.AUTO_REUSE if V.get_store().frozen else None):
        gamma = V.get_variable('gamma', [c], initializer=V.constant_initializer(1.0), keep_fp32=True)
        beta = V.get_variable('beta', [c], initializer=V.constant_initializer(0.0), keep_fp32=True)
    return ops.group_norm(x, gamma, beta, groups, epsilon, "relu" if relu else None, name=name)


def norm(name, x, lsize=4):
    """Local response normalisation; returns the LRN output (fix for SURVEY Q17)."""
    return ops.lrn(x, lsize, bias=1.0, alpha=0.001 / 9.0, beta=0.75, name=name)


def FC_layer(layer_name, x, out_nodes, act="relu"):
    """Flatten + matmul + bias + ReLU, Xavier init (``:190-208``)."""
    if x.dim() == 4:
        size = x.shape[1] * x.shape[2] * x.shape[3]
    else:
        size = x.shape[-1]
    with V.variable_scope(layer_name):
        w = V.get_variable('weights', [size, out_nodes], initializer=V.xavier_initializer())
        b = V.get_variable('biases', [out_nodes], initializer=V.constant_initializer(0.0))
        flat_x = x.reshape(-1, size)
        return ops.dense(flat_x, w, b, act=act)


def weight(kernel_shape, is_uniform=True):
    """Bare Xavier ``weights`` variable in the current scope (``:211-216``)."""
    return V.get_variable('weights', kernel_shape, initializer=V.xavier_initializer(uniform=is_uniform))


def bias(bias_shape):
    """Bare zero-initialised ``biases`` variable (``:219-224``)."""
    return V.get_variable('biases', bias_shape, initializer=V.constant_initializer(0.0))


# ---------------------------------------------------------------------------
# Layers used by the model zoo (ResNet / BERT), same variable conventions.
# ---------------------------------------------------------------------------


def conv_bn(layer_name, x, out_channels, kernel_size=3, stride=1, relu=True, residual=None, training=True,
            bn_decay=0.9, bn_epsilon=1e-5, zero_gamma=False, padding=None, defer=False, pool=None, on_consumer=False,
            groups=1):
    """conv (no bias) → BN (→ +residual) (→ ReLU), ResNet v1.5 building unit.

    Stride>1 convs use TF-official "fixed padding" (symmetric ``(k-1)//2``).  ``defer``: the BN may be
    returned unapplied (``ops.bn.DeferredBN``) for the residual BN that adds it to apply (GPU training).
    ``pool = (ksize, stride, padding)``: a max pool after the ReLU (fused with the BN on the GPU).
    ``on_consumer``: the output's only reader is a 1x1 conv, which may apply the BN + ReLU itself (GPU training).
    ``groups`` above 1: a grouped conv with the filter ``[k, k, Cin / groups, Cout]`` (fan-in from ``Cin / groups``),
    followed by the BN on its own statistics pass; ``defer`` and ``on_consumer`` are ignored.
    """
    variables = conv_bn_variables(layer_name, x, out_channels, kernel_size, zero_gamma=zero_gamma, groups=groups)
    return conv_bn_apply(x, variables, kernel_size, stride, relu, residual, training, bn_decay, bn_epsilon, padding,
                         defer, pool, on_consumer, groups)


def conv_bn_apply(x, variables, kernel_size=3, stride=1, relu=True, residual=None, training=True, bn_decay=0.9,
                  bn_epsilon=1e-5, padding=None, defer=False, pool=None, on_consumer=False, groups=1):
    """:func:`conv_bn` on variables already made by :func:`conv_bn_variables`."""
    k = kernel_size
    if padding is None:
        padding = "SAME" if stride == 1 else ((k - 1) // 2, (k - 1) // 2)
    w, gamma, beta, mm, mv = variables
    return ops.conv_bn(x, w, gamma, beta, mm, mv, stride, padding, training, bn_decay, bn_epsilon, relu, residual,
                       defer=defer, pool=pool, on_consumer=on_consumer, groups=groups)


def conv_bn_variables(layer_name, x, out_channels, kernel_size=3, zero_gamma=False, groups=1, **unused):
    """The variables of :func:`conv_bn` (created on first use, reused after): weights ``[k, k, Cin / groups, Cout]``,
    gamma, beta, moving mean / variance."""
    k = kernel_size
    if x.shape[-1] % groups or out_channels % groups:
        raise ValueError("conv_bn: groups=%d must divide %d and %d channels" % (groups, x.shape[-1], out_channels))
    with V.variable_scope(layer_name):
        w = V.get_variable('weights', [k, k, x.shape[-1] // groups, out_channels],
                           initializer=V.variance_scaling_initializer())
        c = out_channels
        gamma = V.get_variable('BatchNorm/gamma', [c], initializer=V.constant_initializer(0.0 if zero_gamma else 1.0),
                               keep_fp32=True)
        beta = V.get_variable('BatchNorm/beta', [c], initializer=V.constant_initializer(0.0), keep_fp32=True)
        mm = V.get_variable('BatchNorm/moving_mean', [c], initializer=V.constant_initializer(0.0), trainable=False)
        mv = V.get_variable('BatchNorm/moving_variance', [c], initializer=V.constant_initializer(1.0),
                            trainable=False)
    return w, gamma, beta, mm, mv


def dense(layer_name, x, out_features, act=None, initializer=None):
    with V.variable_scope(layer_name):
        w = V.get_variable('kernel', [x.shape[-1], out_features],
                           initializer=initializer or V.truncated_normal_initializer(stddev=0.02))
        b = V.get_variable('bias', [out_features], initializer=V.constant_initializer(0.0))
        shp = x.shape
        y = ops.dense(x.reshape(-1, shp[-1]), w, b, act=act)
        return y.reshape(*shp[:-1], out_features)


def lstm(layer_name, x, num_units, forget_bias=1.0, time_major=False, initial_state=None, sequence_length=None):
    """One LSTM layer over ``x`` [B, T, I] (``time_major``: [T, B, I]): ``(outputs, LSTMStateTuple(c, h))`` with the
    variables ``<layer_name>/lstm_cell/kernel`` and ``.../bias``.  Stack layers by calling it again on the outputs.
    ``sequence_length`` [B]: past its length a row emits zeros and keeps its state."""
    cell = ops.rnn_cell.LSTMCell(num_units, forget_bias=forget_bias)
    return ops.dynamic_rnn(cell, x, sequence_length=sequence_length, initial_state=initial_state,
                           time_major=time_major, scope=layer_name)


def _gru_direction(scope, xt, num_units, initial_state):
    """``(gates kernel, gates bias, candidate kernel, candidate bias, h0)`` of a GRU over time-major ``xt`` with its
    variables under ``scope``."""
    cell = ops.rnn_cell.GRUCell(num_units)
    with V.variable_scope(scope):
        params = cell.variables(xt.shape[2])
    if initial_state is None:
        initial_state = cell.zero_state(xt.shape[1], xt.dtype, device=xt.device)
    return params + (initial_state,)


def gru(layer_name, x, num_units, time_major=False, initial_state=None, sequence_length=None, reverse=False):
    """One GRU layer over ``x`` [B, T, I] (``time_major``: [T, B, I]): ``(outputs, state [B, num_units])`` with the
    variables ``<layer_name>/gru_cell/gates/{kernel,bias}`` and ``.../candidate/{kernel,bias}``.  Stack layers by
    calling it again on the outputs.  ``sequence_length`` [B]: past its length a row emits zeros and keeps its state.
    ``reverse``: row b is read from ``sequence_length[b] - 1`` down to 0; the outputs stay in the time order of ``x``."""
    if not reverse:
        return ops.dynamic_rnn(ops.rnn_cell.GRUCell(num_units), x, sequence_length=sequence_length,
                               initial_state=initial_state, time_major=time_major, scope=layer_name)
    from ..ops import gru as G
    xt = x if time_major else x.transpose(0, 1).contiguous()
    hs, h_t = G.gru(xt, *_gru_direction(layer_name, xt, num_units, initial_state), sequence_length, reverse=True)
    return (hs if time_major else hs.transpose(0, 1)), h_t


def bigru(layer_name, x, num_units, time_major=False, sequence_length=None):
    """One bidirectional GRU layer over ``x``: ``(outputs, (state_fw, state_bw))``, the outputs of the two directions
    concatenated to ``2 * num_units`` features, with the variables
    ``<layer_name>/fw/gru_cell/{gates,candidate}/{kernel,bias}`` and ``<layer_name>/bw/...``, the names TF's
    ``bidirectional_dynamic_rnn`` gives them."""
    from ..ops import gru as G
    xt = x if time_major else x.transpose(0, 1).contiguous()
    with V.variable_scope(layer_name):
        fw, bw = (_gru_direction(d, xt, num_units, None) for d in ("fw", "bw"))
    (hs_fw, h_fw), (hs_bw, h_bw) = G.bigru(xt, fw, bw, sequence_length)
    out = torch.cat([hs_fw, hs_bw], -1)
    return (out if time_major else out.transpose(0, 1)), (h_fw, h_bw)


def bilstm(layer_name, x, num_units, forget_bias=1.0, time_major=False, sequence_length=None):
    """One bidirectional LSTM layer over ``x``: ``(outputs, (state_fw, state_bw))``, the outputs of the two directions
    concatenated to ``2 * num_units`` features, with the variables ``<layer_name>/fw/lstm_cell/{kernel,bias}`` and
    ``<layer_name>/bw/...``."""
    cells = [ops.rnn_cell.LSTMCell(num_units, forget_bias=forget_bias) for _ in range(2)]
    outs, states = ops.bidirectional_dynamic_rnn(cells[0], cells[1], x, sequence_length=sequence_length,
                                                 time_major=time_major, scope=layer_name)
    return torch.cat(outs, -1), states


def attention_layer(layer_name, from_tensor, to_tensor, num_heads, size_per_head, to_lengths=None,
                    attention_mask=None, dropout=0.0, causal=False):
    """BERT's ``attention_layer``: multi-head attention of ``from_tensor`` [B, F, W] over ``to_tensor`` [B, T, W'],
    returning the context [B, F, num_heads * size_per_head] (no output projection).  Variables ``query/kernel``,
    ``query/bias``, ``key/...``, ``value/...`` under ``layer_name``.

    ``to_tensor is from_tensor`` without ``to_lengths``: self-attention, one fused q | k | v projection and
    ``fused_attention`` (``causal`` passed through).  Otherwise encoder-decoder attention: a query projection, one
    fused key | value projection and ``cross_attention``, item b restricted to its first ``to_lengths[b]`` positions
    of ``to_tensor``; ``causal`` has no meaning between two sequences and raises.
    ``attention_mask``: additive [B, T] key mask or None.  ``dropout`` applies while training only."""
    from ..ops import transformer as T
    from ..train import step as S
    self_attention = to_tensor is from_tensor and to_lengths is None
    if causal and not self_attention:
        raise ValueError("attention_layer: causal=True needs to_tensor is from_tensor and no to_lengths")
    B, F_ = from_tensor.shape[0], from_tensor.shape[1]
    T_ = to_tensor.shape[1]
    H = num_heads * size_per_head
    ws, bs = {}, {}
    with V.variable_scope(layer_name):
        # created value, key, query: the flat parameter space lays variables out in reverse creation order, so the
        # biases of a fused projection end up adjacent in q | k | v order (models/bert.py)
        for nm, src in (("value", to_tensor), ("key", to_tensor), ("query", from_tensor)):
            with V.variable_scope(nm):
                ws[nm] = V.get_variable('kernel', [src.shape[-1], H],
                                        initializer=V.truncated_normal_initializer(stddev=0.02))
                bs[nm] = V.get_variable('bias', [H], initializer=V.constant_initializer(0.0))
    drop = dropout if S.is_training() else 0.0
    x = from_tensor.reshape(B * F_, from_tensor.shape[-1])
    if self_attention:
        order = ("query", "key", "value")
        qkv = ops.dense_multi(x, [ws[n] for n in order], [bs[n] for n in order]).reshape(B * F_, 3 * H)
        ctx = T.fused_attention(qkv, B, F_, num_heads, attention_mask, drop, causal=causal)
    else:
        q = ops.dense(x, ws["query"], bs["query"]).reshape(B * F_, H)
        y = to_tensor.reshape(B * T_, to_tensor.shape[-1])
        kv = ops.dense_multi(y, [ws["key"], ws["value"]], [bs["key"], bs["value"]]).reshape(B * T_, 2 * H)
        ctx = T.cross_attention(q, kv, B, F_, T_, num_heads, attention_mask, to_lengths, drop)
    return ctx.reshape(B, F_, H)


def layer_norm(layer_name, x, epsilon=1e-12):
    with V.variable_scope(layer_name):
        g = V.get_variable('gamma', [x.shape[-1]], initializer=V.constant_initializer(1.0), keep_fp32=True)
        b = V.get_variable('beta', [x.shape[-1]], initializer=V.constant_initializer(0.0), keep_fp32=True)
        return ops.layer_norm(x, g, b, epsilon)
