"""``tf.nn.rnn_cell``, ``tf.nn.dynamic_rnn`` and ``tf.nn.bidirectional_dynamic_rnn`` for the LSTM of ``ops/rnn.py`` and
the GRU of ``ops/gru.py`` (``mdtf.nn.rnn_cell``, ``mdtf.nn.dynamic_rnn``, ``mdtf.nn.bidirectional_dynamic_rnn``).

A cell owns no tensors: ``dynamic_rnn`` creates ``<scope or "rnn">/lstm_cell/kernel`` [I + H, 4H] and ``.../bias``
[4H] on first use -- TF's names and layout (gate order i, j, f, o; the input rows first), so a ``Saver`` bundle matches
-- and runs the whole sequence through :func:`mdtf.ops.rnn.lstm`, ``sequence_length`` included; a ``GRUCell`` gets
``.../gru_cell/gates/{kernel,bias}`` [I + H, 2H] / [2H] (r then u) and ``.../gru_cell/candidate/{kernel,bias}``
[I + H, H] / [H] and runs through :func:`mdtf.ops.gru.gru`, ``sequence_length`` included.
``bidirectional_dynamic_rnn`` runs LSTM cells under ``<scope or "bidirectional_rnn">/fw`` and ``.../bw`` through
:func:`mdtf.ops.rnn.bilstm`; it refuses GRU cells, whose two-direction form is :func:`mdtf.ops.gru.bigru` /
``mdtf.layers.tools.bigru``.  Peepholes, projection and cell clipping are not implemented; nor are vanilla cells,
``MultiRNNCell`` (stack layers by calling ``dynamic_rnn`` under different scopes) and dropout wrappers.
"""
import collections

import torch

LSTMStateTuple = collections.namedtuple("LSTMStateTuple", ("c", "h"))


class LSTMCell(object):
    """``tf.nn.rnn_cell.LSTMCell(num_units, forget_bias=1.0)``; ``initializer`` fills the kernel (default: Xavier
    uniform, as TF's), the bias starts at zero."""

    def __init__(self, num_units, forget_bias=1.0, name=None, use_peepholes=False, cell_clip=None, initializer=None,
                 num_proj=None, state_is_tuple=True):
        for what, on in (("use_peepholes", use_peepholes), ("cell_clip", cell_clip is not None),
                         ("num_proj", num_proj is not None), ("state_is_tuple=False", not state_is_tuple)):
            if on:
                raise NotImplementedError("LSTMCell: %s is not implemented" % what)
        self.num_units = int(num_units)
        self.forget_bias = float(forget_bias)
        self.initializer = initializer
        self.name = name or "lstm_cell"

    @property
    def state_size(self):
        return LSTMStateTuple(self.num_units, self.num_units)

    @property
    def output_size(self):
        return self.num_units

    def zero_state(self, batch_size, dtype=torch.float32, device=None):
        from ..train import variables as V
        device = device if device is not None else V.get_store().device
        z = torch.zeros((batch_size, self.num_units), dtype=dtype, device=device)
        return LSTMStateTuple(z, z.clone())

    def variables(self, input_size):
        """The reads of ``<scope>/<name>/kernel`` and ``.../bias`` (created on first use)."""
        from ..train import variables as V
        h = self.num_units
        with V.variable_scope(self.name):
            kernel = V.get_variable("kernel", [input_size + h, 4 * h],
                                    initializer=self.initializer or V.xavier_initializer())
            bias = V.get_variable("bias", [4 * h], initializer=V.constant_initializer(0.0))
        return kernel, bias


BasicLSTMCell = LSTMCell      # the same cell; its variables are named ``lstm_cell`` too unless ``name`` says otherwise


class GRUCell(object):
    """``tf.nn.rnn_cell.GRUCell(num_units)``: the reset gate is applied before the candidate product.
    ``kernel_initializer`` fills both kernels (default: Xavier uniform, as TF's); ``bias_initializer`` fills the
    candidate bias (default 0) and, where given, the gates bias, which otherwise starts at 1.0 as TF's does."""

    def __init__(self, num_units, activation=None, kernel_initializer=None, bias_initializer=None, name=None):
        if activation is not None and activation not in (torch.tanh, "tanh"):
            raise NotImplementedError("GRUCell: only the tanh activation is implemented")
        self.num_units = int(num_units)
        self.kernel_initializer = kernel_initializer
        self.bias_initializer = bias_initializer
        self.name = name or "gru_cell"

    @property
    def state_size(self):
        return self.num_units

    @property
    def output_size(self):
        return self.num_units

    def zero_state(self, batch_size, dtype=torch.float32, device=None):
        from ..train import variables as V
        device = device if device is not None else V.get_store().device
        return torch.zeros((batch_size, self.num_units), dtype=dtype, device=device)

    def variables(self, input_size):
        """The reads of ``<scope>/<name>/gates/{kernel,bias}`` and ``.../candidate/{kernel,bias}`` (created on first
        use)."""
        from ..train import variables as V
        h = self.num_units
        out = []
        with V.variable_scope(self.name):
            for part, cols, bias0 in (("gates", 2 * h, 1.0), ("candidate", h, 0.0)):
                with V.variable_scope(part):
                    out.append(V.get_variable("kernel", [input_size + h, cols],
                                              initializer=self.kernel_initializer or V.xavier_initializer()))
                    out.append(V.get_variable("bias", [cols], initializer=self.bias_initializer
                                              or V.constant_initializer(bias0)))
        return tuple(out)



def dynamic_rnn(cell, inputs, sequence_length=None, initial_state=None, dtype=None, time_major=False, scope=None):
    """``tf.nn.dynamic_rnn``: ``(outputs, LSTMStateTuple(c, h))`` for ``inputs`` [B, T, I] (``time_major``: [T, B, I]);
    for a ``GRUCell`` the state is one tensor [B, H], in the dtype of ``inputs``.  Without ``initial_state`` the state
    starts at zero (in ``dtype`` or the dtype of ``inputs``).  On the HIP path the returned ``c`` is fp32."""
    from . import rnn
    from ..train import variables as V
    if not isinstance(cell, (LSTMCell, GRUCell)):
        raise TypeError("dynamic_rnn: only LSTMCell / BasicLSTMCell / GRUCell cells are implemented, got %r" % (cell,))
    if inputs.dim() != 3:
        raise ValueError("dynamic_rnn: inputs must be rank 3, got %s" % (tuple(inputs.shape),))
    x = inputs if time_major else inputs.transpose(0, 1).contiguous()    # the kernels are time-major
    batch = x.shape[1]
    if initial_state is None:
        initial_state = cell.zero_state(batch, dtype or x.dtype, device=x.device)
    if isinstance(cell, GRUCell):
        from . import gru
        with V.variable_scope(scope if scope is not None else "rnn"):
            params = cell.variables(x.shape[2])
        hs, h_t = gru.gru(x, *params, initial_state, sequence_length)
        return (hs if time_major else hs.transpose(0, 1)), h_t
    c0, h0 = initial_state
    with V.variable_scope(scope if scope is not None else "rnn"):
        kernel, bias = cell.variables(x.shape[2])
    hs, h_t, c_t = rnn.lstm(x, kernel, bias, h0, c0, cell.forget_bias, sequence_length)
    return (hs if time_major else hs.transpose(0, 1)), LSTMStateTuple(c_t, h_t)


def bidirectional_dynamic_rnn(cell_fw, cell_bw, inputs, sequence_length=None, initial_state_fw=None,
                              initial_state_bw=None, dtype=None, time_major=False, scope=None):
    """``tf.nn.bidirectional_dynamic_rnn``: ``((out_fw, out_bw), (state_fw, state_bw))``.  ``cell_bw`` reads row b
    from ``sequence_length[b] - 1`` down to 0 and ``out_bw`` is in the time order of ``inputs``; past its length a row
    is zero in both.  Variables: ``<scope or "bidirectional_rnn">/fw/lstm_cell/{kernel,bias}`` and ``.../bw/...``.
    LSTM cells only: ``GRUCell``s raise ``TypeError`` here, and a forward plus a reverse GRU in the same launches is
    :func:`mdtf.ops.gru.bigru` (``mdtf.layers.tools.bigru`` with TF's variable names)."""
    from . import rnn
    from ..train import variables as V
    for cell in (cell_fw, cell_bw):
        if not isinstance(cell, LSTMCell):
            raise TypeError("bidirectional_dynamic_rnn: only LSTMCell / BasicLSTMCell cells are implemented, got %r"
                            % (cell,))
    if inputs.dim() != 3:
        raise ValueError("bidirectional_dynamic_rnn: inputs must be rank 3, got %s" % (tuple(inputs.shape),))
    x = inputs if time_major else inputs.transpose(0, 1).contiguous()
    params = []
    with V.variable_scope(scope if scope is not None else "bidirectional_rnn"):
        for name, cell, state in (("fw", cell_fw, initial_state_fw), ("bw", cell_bw, initial_state_bw)):
            if state is None:
                state = cell.zero_state(x.shape[1], dtype or x.dtype, device=x.device)
            c0, h0 = state
            with V.variable_scope(name):
                params.append(cell.variables(x.shape[2]) + (h0, c0))
    res = rnn.bilstm(x, params[0], params[1], (cell_fw.forget_bias, cell_bw.forget_bias), sequence_length)
    outs = tuple(hs if time_major else hs.transpose(0, 1) for hs, _, _ in res)
    return outs, tuple(LSTMStateTuple(c_t, h_t) for _, h_t, c_t in res)
