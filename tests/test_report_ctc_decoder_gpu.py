"""``ReportCTCDecoder`` on the device path (``CTCGreedyDecoder.launch_device`` -> ``wer.DeviceWordErrorRate`` ->
``ms_edit_distance``) against the host path and against ``wer.WordErrorRate``: the same ``wer`` float, the same transcripts.
Equality throughout."""
import pytest
import torch

from myrtlespeech_amd.data.alphabet import Alphabet
from myrtlespeech_amd.post_process.ctc_beam_decoder import CTCBeamDecoder
from myrtlespeech_amd.post_process.ctc_greedy_decoder import CTCGreedyDecoder
from myrtlespeech_amd.run.callbacks import Callback, CallbackHandler, ReportCTCDecoder, ReportMeanBatchLoss
from myrtlespeech_amd.wer import DeviceWordErrorRate, WordErrorRate, WordSegmentor

pytestmark = pytest.mark.gpu

T_, N, V = 40, 5, 12
ALPHABET = Alphabet(list(" abcdefghij"))          # 11 symbols, the separator is label 0, the blank label 11
BLANK = V - 1


def batches():
    """Two eval batches: logits [T, N, V] with frame counts, targets with one row that holds no word."""
    gen = torch.Generator().manual_seed(11)
    out = []
    for b in range(2):
        logits = torch.randn(T_, N, V, generator=gen) * 3
        logits[:, :, 0] += 1.5                                                    # enough separators for several words
        lens = torch.tensor([40, 33, 40, 7, 1][b:] + [21] * b)
        targets = torch.randint(0, V - 1, (N, 9), generator=gen, dtype=torch.int32)
        targets[1, :] = 0                                                         # separators only: an empty word list
        target_lens = torch.tensor([9, 4, 6, 0, 1], dtype=torch.int32)
        out.append(((logits, lens), (targets, target_lens)))
    return out


def run_eval(cb, data, on_gpu_targets=False):
    handler = CallbackHandler([cb])
    handler.on_train_begin(1)
    handler.train(False)
    handler.on_epoch_begin()
    for (logits, lens), (targets, target_lens) in data:
        y = (targets.cuda(), target_lens.cuda()) if on_gpu_targets else (targets, target_lens)
        handler.on_batch_begin("x", y)
        handler.on_loss_begin((logits.cuda(), lens), y)
        handler.on_batch_end()
    handler.on_epoch_end()
    return handler.state_dict["reports"]


def host_wer(decoder, data):
    wer = WordErrorRate(ALPHABET, WordSegmentor(" "))
    for (logits, lens), (targets, target_lens) in data:
        wer.update(decoder(logits.cuda(), lens), targets, target_lens)
    return wer


def test_launch_device_equals_forward():
    dec = CTCGreedyDecoder(BLANK)
    for (logits, lens), _ in batches():
        labels, label_lens = dec.launch_device(logits.cuda(), lens)
        assert labels.is_cuda and labels.dtype == torch.int32 and labels.shape == (N, T_)
        assert label_lens.is_cuda and label_lens.dtype == torch.int32 and label_lens.shape == (N,)
        got = [labels[n, :int(label_lens[n])].tolist() for n in range(N)]
        assert got == dec(logits.cuda(), lens)
    labels, label_lens = dec.launch_device(torch.zeros(0, 2, V), torch.tensor([0, 0]))
    assert labels.shape == (2, 0) and label_lens.tolist() == [0, 0]


def test_device_path_equals_host_path_and_word_error_rate():
    data = batches()
    dec = CTCGreedyDecoder(BLANK)
    want = host_wer(dec, data)
    assert any(not exp for _, exp in want.transcripts) and sum(want.distances) > 0 and len(want.transcripts) == 2 * N
    host = run_eval(ReportCTCDecoder(dec, ALPHABET, WordSegmentor(" "), on_device=False), data)["CTCGreedyDecoder"]
    assert host == {"wer": want.value(), "transcripts": want.transcripts}
    for on_gpu_targets in (False, True):
        cb = ReportCTCDecoder(dec, ALPHABET, WordSegmentor(" "), on_device=True)
        device = run_eval(cb, data, on_gpu_targets)["CTCGreedyDecoder"]
        assert device["wer"] == want.value()
        assert device["transcripts"] == want.transcripts
        counts = cb.device_wer.counts()
        assert counts.distance == sum(want.distances) and counts.ref_units == sum(want.lengths)
        assert counts.hyp_units == sum(len(act) for act, _ in want.transcripts)
        assert counts.substitutions + counts.deletions + counts.insertions == counts.distance
    # the default takes the device path for this alphabet
    assert run_eval(ReportCTCDecoder(dec, ALPHABET, WordSegmentor(" ")), data)["CTCGreedyDecoder"] == host


def test_without_transcripts_only_the_rate_is_reported():
    data = batches()
    dec = CTCGreedyDecoder(BLANK)
    cb = ReportCTCDecoder(dec, ALPHABET, WordSegmentor(" "), on_device=True, keep_transcripts=False)
    got = run_eval(cb, data)["CTCGreedyDecoder"]
    assert got == {"wer": host_wer(dec, data).value(), "transcripts": []}


def test_token_unit_and_a_separator_outside_the_alphabet():
    data = batches()
    dec = CTCGreedyDecoder(BLANK)
    tokens = DeviceWordErrorRate(ALPHABET, WordSegmentor(" "), unit="token")
    one_word = DeviceWordErrorRate(ALPHABET, WordSegmentor("#"))
    want_words = WordErrorRate(ALPHABET, WordSegmentor("#"))
    distance = length = 0
    from myrtlespeech_amd.post_process.utils import levenshtein
    for (logits, lens), (targets, target_lens) in data:
        hyp = dec(logits.cuda(), lens)
        tokens.update(dec.launch_device(logits.cuda(), lens), targets, target_lens)
        one_word.update(hyp, targets.cuda(), target_lens)
        want_words.update(hyp, targets, target_lens)
        for h, t, n in zip(hyp, targets.tolist(), target_lens.tolist()):
            distance += levenshtein(h, t[:n])
            length += n
    assert tokens.value() == float(distance) / length * 100
    assert one_word.value() == want_words.value()


def test_beam_decoder_goes_through_the_upload_path():
    data = [((torch.softmax(logits, dim=2), lens), y) for (logits, lens), y in batches()]
    dec = CTCBeamDecoder(BLANK, beam_width=4)
    want = host_wer(dec, data)
    got = run_eval(ReportCTCDecoder(dec, ALPHABET, WordSegmentor(" "), on_device=True), data)["CTCBeamDecoder"]
    assert got == {"wer": want.value(), "transcripts": want.transcripts}


DS2_TINY = '''
alphabet: " abcdefghi_";
pre_process_step { stage: TRAIN_AND_EVAL; mfcc { n_mfcc: 16; win_length: 400; hop_length: 160; } }
deep_speech_2 {
  conv_block { conv2d { output_channels: 4; kernel_feature: 5; kernel_time: 3; stride_feature: 2; stride_time: 2;
                        padding_mode: SAME; bias: true; } activation { hardtanh { min_val: 0.0; max_val: 20.0; } } }
  conv_block { conv2d { output_channels: 4; kernel_feature: 3; kernel_time: 3; stride_feature: 2; stride_time: 1;
                        padding_mode: SAME; bias: true; } activation { hardtanh { min_val: 0.0; max_val: 20.0; } } }
  rnn { rnn_type: LSTM; hidden_size: 16; num_layers: 2; bias: true; bidirectional: true; forget_gate_bias { value: 1.0 } }
  lookahead_block { no_lookahead {} activation { identity {} } }
  fully_connected { num_hidden_layers: 1; hidden_size: 24; activation { hardtanh { min_val: 0.0; max_val: 20.0; } } }
}
ctc_loss { blank_index: 10; reduction: SUM; }
ctc_greedy_decoder { blank_index: 10; }
'''


def test_fit_reports_the_word_error_rate_after_every_eval_pass():
    """The tiny builder-built DS2 of test_gpu_parity.py's builder test with the reference's weights (so the transcripts are not
    empty), no optimizer (so both EVAL passes see the same model): ``fit`` for one epoch leaves, after each EVAL pass, the rate
    ``WordErrorRate`` gives on the model's own greedy transcripts."""
    from util import Golden

    from myrtlespeech_amd import protos as P
    from myrtlespeech_amd.builders.speech_to_text import build as build_stt
    from myrtlespeech_amd.run.train import fit
    g = Golden("ds2_tiny_bilstm")
    stt = build_stt(P.parse(DS2_TINY, P.SpeechToText))
    stt.model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in g.sd().items()}, strict=True)
    x = (torch.from_numpy(g["in/x"].copy()), torch.from_numpy(g["in/lens"].copy()))
    ys = [(torch.tensor([[1, 2, 0, 3], [4, 0, 5, 0], [6, 0, 0, 0]], dtype=torch.int32), torch.tensor([4, 3, 1], dtype=torch.int32)),
          (torch.tensor([[0, 7, 7, 0], [1, 0, 1, 0], [0, 0, 2, 3]], dtype=torch.int32), torch.tensor([4, 4, 4], dtype=torch.int32))]
    eval_loader = [(x, y) for y in ys]
    seen = []

    class Keep(Callback):
        def on_epoch_end(self, **kwargs):
            if not self.training:
                seen.append({k: (dict(v) if isinstance(v, dict) else v) for k, v in kwargs["reports"].items()})

    report = ReportCTCDecoder(stt.post_process, stt.alphabet, WordSegmentor(" "))
    assert report.on_device
    fit(stt, 1, [(x, ys[0])], eval_loader=eval_loader, callbacks=[ReportMeanBatchLoss(), report, Keep()])
    stt.eval()
    want = WordErrorRate(stt.alphabet, WordSegmentor(" "))
    with torch.no_grad():
        (out, out_lens), _ = stt.model(x)
    hyp = stt.post_process(out, out_lens)
    assert any(hyp)
    for y in ys:
        want.update(hyp, *y)
    assert len(seen) == 2
    for reports in seen:
        assert reports["CTCGreedyDecoder"] == {"wer": want.value(), "transcripts": want.transcripts}
        assert isinstance(reports["ReportMeanBatchLoss"], float)
