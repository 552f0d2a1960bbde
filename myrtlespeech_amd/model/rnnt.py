"""RNN-T (transducer) modules -- this repository's OWN specification.

The reference snapshot contains no transducer, so nothing here mirrors a
reference file; BASELINE.json's configs[3] names the shape (DS2 encoder + 2-layer LSTM
predictor + joint network, beam width 8).  Specification (Graves 2012, "Sequence Transduction
with Recurrent Neural Networks"):

* encoder: any module returning ``((enc[T', N, E], lens), hid)`` -- normally ``DeepSpeech2``;
* ``RNNTPredictor``: ``Embedding(V + 1, D)`` (index ``V`` = blank = start-of-sequence) followed by
  an ``L``-layer unidirectional LSTM (``model.rnn.RNN``);
* ``RNNTJoint``: ``log_softmax(out(tanh(enc_proj(enc_t) + pred_proj(pred_u))))`` over ``V + 1``
  symbols, blank last.
"""
from typing import Optional, Tuple

import torch

from myrtlespeech_amd import _lib
from myrtlespeech_amd.model.rnn import RNN, RNNType


class RNNTPredictor(torch.nn.Module):
    def __init__(self, vocab_size: int, embed_dim: int, hidden_size: int, num_layers: int = 2):
        super().__init__()
        self.vocab_size = vocab_size
        self.blank = vocab_size
        self.embedding = torch.nn.Embedding(vocab_size + 1, embed_dim)  # parameter container
        self.rnn = RNN(RNNType.LSTM, embed_dim, hidden_size, num_layers=num_layers)
        self.hidden_size = hidden_size
        self.num_layers = num_layers
        if torch.cuda.is_available():
            self.cuda()

    def zero_state(self, rows: int):
        z = torch.zeros(self.num_layers, rows, self.hidden_size, device="cuda")
        return z, z.clone()

    def step(self, labels: torch.Tensor, state: Tuple[torch.Tensor, torch.Tensor]):
        """labels [R] int (device) -> (pred_out [R, hidden], new_state); one symbol per row."""
        _lib.require_gpu()
        r = labels.numel()
        w = _lib.f32c(self.embedding.weight.detach())
        idx = labels.to(device="cuda", dtype=torch.int32).contiguous()
        emb = torch.empty((1, r, w.shape[1]), dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().ms_embedding_forward(_lib.ptr(w), _lib.ptr(idx), _lib.ptr(emb), r, w.shape[1], w.shape[0],
                                                    _lib.stream_ptr()), "ms_embedding_forward")
        (out, _), new_state = self.rnn((emb, torch.ones(r, dtype=torch.int64)), state)
        return out[0], new_state

    def forward_targets(self, targets: torch.Tensor, target_lens: torch.Tensor, differentiable: bool = False) -> torch.Tensor:
        """targets [N, U] padded labels -> pred [U + 1, N, hidden]: row u is the prediction after ``y_n[:u]`` (u = 0: after
        the start symbol), for GIVEN transcripts.  ONE embedding look-up over ``[blank, y_0 .. y_{U-1}]`` of the whole batch
        (time-major rows) and ONE call of the recurrent stack on the [U + 1, N, D] sequence from a zero state, where ``step``
        (kept for the decoders) would take U + 1 rounds.  The predictor is causal, so what the padding of ``targets`` holds
        (the look-up clamps it) only reaches rows u > target_lens[n]; ``target_lens`` is checked against the batch only.
        Detached by default.  ``differentiable=True``: the same look-up and the same stack as autograd nodes
        (``model.rnn_autograd``: ``embedding_train``, ``lstm_train``), so a gradient of ``pred`` reaches the embedding table
        and every LSTM parameter."""
        if targets.dim() != 2 or targets.is_floating_point():
            raise ValueError(f"targets must be an integer tensor [N, U], got {tuple(targets.shape)} {targets.dtype}")
        n, u_max = targets.shape
        if n <= 0 or target_lens.numel() != n:
            raise ValueError(f"target lengths of batch {target_lens.numel()} != targets batch {n}")
        _lib.require_gpu()
        y = targets.detach().to(device="cuda", dtype=torch.int32)
        idx = torch.cat([torch.full((1, n), self.blank, dtype=torch.int32, device="cuda"), y.t()], 0).contiguous()
        if differentiable:
            from myrtlespeech_amd.model.rnn_autograd import embedding_train, lstm_train
            emb = embedding_train(self.embedding.weight, idx)                   # [U + 1, N, D]
            out, _ = lstm_train(self.rnn, emb, torch.full((n,), u_max + 1, dtype=torch.int64))
            return out
        w = _lib.f32c(self.embedding.weight.detach())
        rows = (u_max + 1) * n
        emb = torch.empty((u_max + 1, n, w.shape[1]), dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().ms_embedding_forward(_lib.ptr(w), _lib.ptr(idx), _lib.ptr(emb), rows, w.shape[1], w.shape[0],
                                                    _lib.stream_ptr()), "ms_embedding_forward")
        (out, _), _ = self.rnn((emb, torch.full((n,), u_max + 1, dtype=torch.int64)), self.zero_state(n))
        return out


class RNNTJoint(torch.nn.Module):
    def __init__(self, enc_features: int, pred_features: int, joint_features: int, vocab_size: int):
        super().__init__()
        self.enc_proj = torch.nn.Linear(enc_features, joint_features)
        self.pred_proj = torch.nn.Linear(pred_features, joint_features, bias=False)
        self.out = torch.nn.Linear(joint_features, vocab_size + 1)
        self.vocab_size = vocab_size
        if torch.cuda.is_available():
            self.cuda()

    @staticmethod
    def _linear(x2d: torch.Tensor, lin: torch.nn.Linear) -> torch.Tensor:
        lib = _lib.load()
        m, k = x2d.shape
        y = torch.empty((m, lin.out_features), dtype=torch.float32, device="cuda")
        w = _lib.f32c(lin.weight.detach())
        b = None if lin.bias is None else _lib.f32c(lin.bias.detach())
        _lib.check(lib.ms_linear_forward(_lib.ptr(x2d), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), m, k, lin.out_features,
                                         _lib.ACT_NONE, 0.0, 0.0, _lib.stream_ptr()), "ms_linear_forward")
        return y

    def project_encoder(self, enc: torch.Tensor, differentiable: bool = False) -> torch.Tensor:
        """enc [T, N, E] -> [T*N, J] (done once per batch).  ``differentiable=True``: as an autograd node
        (``model.rnn_autograd.linear_train``) whose gradients reach ``enc_proj`` and ``enc``."""
        if differentiable:
            if enc.dim() != 3 or enc.shape[2] != self.enc_proj.in_features:
                raise ValueError(f"enc must be [T, N, {self.enc_proj.in_features}], got {tuple(enc.shape)}")
            _lib.require_gpu()
            from myrtlespeech_amd.model.rnn_autograd import linear_train
            return linear_train(enc.reshape(enc.shape[0] * enc.shape[1], enc.shape[2]), self.enc_proj)
        t, n, e = enc.shape
        return self._linear(_lib.f32c(enc).reshape(t * n, e), self.enc_proj)

    def project_predictor(self, pred: torch.Tensor, differentiable: bool = False) -> torch.Tensor:
        """pred [U + 1, N, H] (``RNNTPredictor.forward_targets``) -> [(U + 1)*N, J].  ``differentiable=True``: as an autograd
        node whose gradients reach ``pred_proj`` and ``pred``."""
        if pred.dim() != 3 or pred.shape[2] != self.pred_proj.in_features:
            raise ValueError(f"pred must be [U + 1, N, {self.pred_proj.in_features}], got {tuple(pred.shape)}")
        _lib.require_gpu()
        rows = pred.shape[0] * pred.shape[1]
        if differentiable:
            from myrtlespeech_amd.model.rnn_autograd import linear_train
            return linear_train(pred.reshape(rows, pred.shape[2]), self.pred_proj)
        return self._linear(_lib.f32c(pred).reshape(rows, -1), self.pred_proj)

    def logprobs(self, enc_p: torch.Tensor, enc_rows: torch.Tensor, pred_out: torch.Tensor) -> torch.Tensor:
        """log P(symbol | frame, prefix) for R hypothesis rows: enc_rows [R] indexes rows of ``enc_p``."""
        r = pred_out.shape[0]
        pred_p = self._linear(_lib.f32c(pred_out), self.pred_proj)
        rows = enc_rows.to(device="cuda", dtype=torch.int32).contiguous()
        w = _lib.f32c(self.out.weight.detach())
        b = _lib.f32c(self.out.bias.detach())
        logp = torch.empty((r, w.shape[0]), dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().ms_rnnt_joint_forward(_lib.ptr(enc_p), _lib.ptr(rows), _lib.ptr(pred_p), _lib.ptr(w),
                                                     _lib.ptr(b), _lib.ptr(logp), r, w.shape[1], w.shape[0],
                                                     _lib.stream_ptr()), "ms_rnnt_joint_forward")
        return logp


class RNNT(torch.nn.Module):
    """Encoder + prediction network + joint network."""

    def __init__(self, encoder: torch.nn.Module, predictor: RNNTPredictor, joint: RNNTJoint):
        super().__init__()
        self.encoder = encoder
        self.predictor = predictor
        self.joint = joint

    def encode(self, x: Tuple[torch.Tensor, torch.Tensor], hx: Optional[object] = None):
        (enc, lens), _ = self.encoder(x, hx)
        return enc, lens

    def joint_lattice(self, enc: torch.Tensor, lens: torch.Tensor, targets: torch.Tensor, target_lens: torch.Tensor
                      ) -> torch.Tensor:
        """The joint's log-probabilities for GIVEN transcripts: enc [T, N, E] encoder frames, targets [N, U] padded labels ->
        [N, T, U + 1, V + 1], row (n, t, u) = log P(symbol | frame t, y_n[:u]) -- what ``loss.rnnt_loss.RNNTLoss`` takes, so
        ``RNNTLoss(blank=V, reduction="none")((lattice, lens), (targets, target_lens))`` is -log P(transcript | audio).
        Built from the decoders' pieces only (``predictor.step`` over blank and then the labels, ``joint.project_encoder``,
        ``joint.logprobs``) and detached: it serves scoring, not training.  The predictor is causal, so what the padding of
        ``targets`` holds (the embedding look-up clamps it) only reaches rows u > target_lens[n], which the loss never reads;
        ``lens`` / ``target_lens`` are checked against the shapes and otherwise left to the loss.
        This materialises N T (U + 1) (V + 1) floats in U + 1 rounds of small launches: for small alphabets and short
        transcripts only.  ``transcript_nll`` gives the same -log P without the lattice."""
        _lib.require_gpu()
        if enc.dim() != 3 or targets.dim() != 2 or targets.shape[0] != enc.shape[1]:
            raise ValueError(f"enc must be [T, N, E] and targets [N, U], got {tuple(enc.shape)} and {tuple(targets.shape)}")
        t, n, _ = enc.shape
        u_max = targets.shape[1]
        if lens.numel() != n or target_lens.numel() != n:
            raise ValueError(f"lengths of batch {lens.numel()} / {target_lens.numel()} != encoder batch {n}")
        with torch.no_grad():
            enc_p = self.joint.project_encoder(enc.detach())                    # [T*N, J], row t*N + n
            y = targets.detach().to(device="cuda", dtype=torch.int32)
            labels = torch.full((n,), self.predictor.blank, dtype=torch.int32, device="cuda")
            state = self.predictor.zero_state(n)
            enc_rows = torch.arange(t * n, dtype=torch.int32, device="cuda")
            out = torch.empty((n, t, u_max + 1, self.joint.vocab_size + 1), dtype=torch.float32, device="cuda")
            for u in range(u_max + 1):
                pred, state = self.predictor.step(labels, state)                # [N, H]: the prediction after y[:u]
                logp = self.joint.logprobs(enc_p, enc_rows, pred.repeat(t, 1))  # row t*N + n pairs frame t with utterance n
                out[:, :, u, :] = logp.reshape(t, n, -1).transpose(0, 1)
                if u < u_max:
                    labels = y[:, u].contiguous()
        return out

    def transcript_nll(self, enc: torch.Tensor, lens: torch.Tensor, targets: torch.Tensor, target_lens: torch.Tensor
                       ) -> torch.Tensor:
        """-log P(transcript | audio) per utterance, [N] float32 on the device, WITHOUT the logit lattice: enc [T, N, E]
        encoder frames, targets [N, U] padded labels.  The same quantity as ``RNNTLoss(blank=V, reduction="none")`` on
        ``joint_lattice`` (up to the bounds of tests/test_rnnt_score_gpu.py), from one projection of the encoder, one pass of
        the predictor over the transcripts (``forward_targets``), one projection of its output and ``loss.rnnt_loss.rnnt_score``,
        whose memory does not grow with the alphabet.  Detached: it serves scoring, not training."""
        from myrtlespeech_amd.loss.rnnt_loss import check_score_shapes, rnnt_score
        if enc.dim() != 3 or targets.dim() != 2 or targets.shape[0] != enc.shape[1]:
            raise ValueError(f"enc must be [T, N, E] and targets [N, U], got {tuple(enc.shape)} and {tuple(targets.shape)}")
        t, n, _ = enc.shape
        u1 = targets.shape[1] + 1
        w, b = self.joint.out.weight, self.joint.out.bias
        blank = self.predictor.blank
        check_score_shapes(t, n, u1, w.shape[1], w.shape[0], lens, targets, target_lens, blank)
        _lib.require_gpu()
        with torch.no_grad():
            enc_p = self.joint.project_encoder(enc.detach())                    # [T*N, J], row t*N + n
            pred = self.predictor.forward_targets(targets, target_lens)         # [U1, N, H]
            pred_p = self.joint._linear(_lib.f32c(pred).reshape(u1 * n, -1), self.joint.pred_proj)   # [U1*N, J], row u*N + n
            return rnnt_score(enc_p.reshape(t, n, -1), pred_p.reshape(u1, n, -1), w.detach(), None if b is None else b.detach(),
                              lens, targets, target_lens, blank)

    def loss(self, enc: torch.Tensor, lens: torch.Tensor, targets: torch.Tensor, target_lens: torch.Tensor,
             reduction: str = "mean") -> torch.Tensor:
        """The transducer loss of GIVEN transcripts as a differentiable call, WITHOUT the logit lattice: the plumbing of
        ``transcript_nll`` with every stage an autograd node -- ``joint.project_encoder``, ``predictor.forward_targets`` and
        ``joint.project_predictor`` with ``differentiable=True``, then ``loss.rnnt_loss.rnnt_joint_loss`` (its reductions:
        ``none`` nll [N], ``sum``, ``mean`` = the sum divided by N).  enc [T, N, E] encoder frames, targets [N, U] padded
        labels.  Gradients reach ``predictor.embedding.weight``, every parameter of the predictor's LSTM, ``joint.enc_proj``,
        ``joint.pred_proj`` and ``joint.out`` -- and ``enc`` itself when it requires grad.  That is where the chain ends: the
        encoder modules (convolutions, bidirectional stacks, GRU) still have no backward in this project, so ``enc`` must be
        a leaf or come from torch ops; this trains or adapts the prediction network and the joint on a frozen encoder."""
        from myrtlespeech_amd.loss.rnnt_loss import _REDUCTIONS, check_score_shapes, rnnt_joint_loss
        if reduction not in _REDUCTIONS:
            raise ValueError(f"{reduction} is not a valid value for reduction")
        if enc.dim() != 3 or targets.dim() != 2 or targets.shape[0] != enc.shape[1]:
            raise ValueError(f"enc must be [T, N, E] and targets [N, U], got {tuple(enc.shape)} and {tuple(targets.shape)}")
        t, n, _ = enc.shape
        u1 = targets.shape[1] + 1
        w, b = self.joint.out.weight, self.joint.out.bias
        blank = self.predictor.blank
        check_score_shapes(t, n, u1, w.shape[1], w.shape[0], lens, targets, target_lens, blank)
        _lib.require_gpu()
        enc_p = self.joint.project_encoder(enc, differentiable=True)                        # [T*N, J], row t*N + n
        pred = self.predictor.forward_targets(targets, target_lens, differentiable=True)     # [U1, N, H]
        pred_p = self.joint.project_predictor(pred, differentiable=True)                    # [U1*N, J], row u*N + n
        return rnnt_joint_loss(enc_p.reshape(t, n, -1), pred_p.reshape(u1, n, -1), w, b, lens, targets, target_lens, blank,
                               reduction)

    def align(self, enc: torch.Tensor, lens: torch.Tensor, targets: torch.Tensor, target_lens: torch.Tensor):
        """Forced alignment of GIVEN transcripts, WITHOUT the logit lattice: enc [T, N, E] encoder frames, targets [N, U]
        padded labels -> one ``post_process.rnnt_aligner.RNNTAlignment`` per utterance (the best path's score, the frame at
        which every label is emitted, each frame's blank log-probability), ``None`` where the transcript cannot be aligned.
        The plumbing of ``transcript_nll`` -- one projection of the encoder, ``forward_targets``, one projection of its output
        -- then ``ms_rnnt_align_joint``: the scorer's pack and cells launches and the aligner's walk, whose memory does not
        grow with the alphabet.  The same path as ``RNNTForcedAligner`` on ``joint_lattice`` wherever the best path leads by
        more than the bounds of tests/test_rnnt_align_gpu.py.  Detached; one staged upload, one read-back."""
        from myrtlespeech_amd.loss.rnnt_loss import _score_inputs, check_score_shapes
        from myrtlespeech_amd.post_process import rnnt_aligner as A
        if enc.dim() != 3 or targets.dim() != 2 or targets.shape[0] != enc.shape[1]:
            raise ValueError(f"enc must be [T, N, E] and targets [N, U], got {tuple(enc.shape)} and {tuple(targets.shape)}")
        t, n, _ = enc.shape
        u1 = targets.shape[1] + 1
        w, b = self.joint.out.weight, self.joint.out.bias
        blank = self.predictor.blank
        xl, yl = check_score_shapes(t, n, u1, w.shape[1], w.shape[0], lens, targets, target_lens, blank)
        labels = A.validate_labels(targets, yl, w.shape[0], blank)
        _lib.require_gpu()
        lib = _lib.load()
        with torch.no_grad():
            enc_p = self.joint.project_encoder(enc.detach())                    # [T*N, J], row t*N + n
            pred = self.predictor.forward_targets(targets, target_lens)         # [U1, N, H]
            pred_p = self.joint._linear(_lib.f32c(pred).reshape(u1 * n, -1), self.joint.pred_proj)   # [U1*N, J], row u*N + n
            args, shape = _score_inputs(enc_p.reshape(t, n, -1), pred_p.reshape(u1, n, -1), w.detach(),
                                        None if b is None else b.detach(), lens, targets, target_lens, blank)
            e, p, wd, bd, xl_dev, y_dev, yl_dev = args
            j, v1 = shape[3], shape[4]
            out, (score, t_frame, t_logp, f_u, f_logp), sizes = A.output_buffer(n, t, u1)
            nbytes = lib.ms_rnnt_align_joint_workspace_bytes(n, t, u1, j, v1)
            ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")     # transient: nothing outlives the call
            has_tokens = u1 > 1
            _lib.check(lib.ms_rnnt_align_joint(_lib.ptr(e), _lib.ptr(p), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(xl_dev),
                                               _lib.ptr(y_dev), _lib.ptr(yl_dev), _lib.ptr(score),
                                               _lib.ptr(t_frame if has_tokens else None),
                                               _lib.ptr(t_logp if has_tokens else None), _lib.ptr(f_u), _lib.ptr(f_logp), n, t,
                                               u1, j, v1, int(blank), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "ms_rnnt_align_joint")
        return A.read_back(out, sizes, labels, xl.tolist(), n, t, u1, "RNNT.align")
