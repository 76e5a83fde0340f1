"""Tacotron inference in front of the vocoder -- BASELINE config 3's caller side (`gen_tacotron.py wavernn`, reference
gen_tacotron.py:139-166; SURVEY.md section 8 row f3's host).

This is NOT the hot path and not a kernel: it is the reference's `Tacotron.generate()` (models/tacotron.py:370-430) restated as
a FUNCTIONAL forward over a reference state dict (`tts_model.state_dict()` / `latest_weights.pyt`), on whatever device the
tensors live on -- PyTorch-ROCm on an MI355X.  No module tree, no training code, eval semantics only (dropout and zoneout
are identities in `generate()`, which calls `self.eval()` first, :371).  On the CPU it reproduces the reference bit for bit
(tests/test_tacotron_mirror.py, build container; tests/golden/tacotron_decoder_200f.npz holds the reference's own output for the
GPU tests' weights); on the GPU the decoder loop -- one sentence = one serial chain of ~40 small ops per mel frame -- runs as ONE
persistent kernel (`generate(..., kernel=True)`: `wrnn_taco_decode`, csrc/wrnn_taco.hip) and the CBHGs'
bidirectional GRUs as `wrnn_bigru`; the eager loop stays as the any-device form.  `generate(..., cbhg_kernel=True)` (opt-in) also runs
the encoder and the post-net -- embedding, pre-net, both CBHGs, `encoder_proj`, `post_proj` -- as HIP kernels through the C ABI
(`wrnn_taco_encode` / `wrnn_taco_postnet`, csrc/wrnn_cbhg.hip), so that the whole Tacotron side is behind include/wavernn_amd.h.
`generate_batch(list_of_ids)` decodes up to eight sentences per pass of the decoder kernel (`wrnn_taco_decode_batch`, csrc/wrnn_taco_batch.hip).
`forward_gta(ids, mel)` / `forward_gta_batch(...)` run the decoder TEACHER-FORCED over a recording's own mel -- the reference's
`Tacotron.forward(x, m, generate_gta=True)` (:310-368), the ground-truth-aligned features its vocoder is trained on -- through
`wrnn_taco_decode_forced` (the same file; `python -m wavernn_amd.gta_tacotron` is the command line).

    tts = TacotronInference(state_dict, device='cuda')
    _, m, attn = tts.generate(ids, steps=800)                 # same returns as the reference: (80, N), (fft, N), (N, chars); the
                                                              # vocoder takes the SECOND one (postnet output; gen_tacotron.py:142)
    m = torch.tensor(np.clip((m + 4) / 8, 0, 1)).unsqueeze(0)     # gen_tacotron.py:143-145
    voc.generate(m, path, True, 11_000, 550, True)               # gen_tacotron.py:161-163
"""
import collections
import re

import numpy as np
import torch
import torch.nn.functional as F

from ._lib import TACO_BATCH_MAX

#: the character part of the reference's symbol table (utils/text/symbols.py:8-17: pad, '-', punctuation, letters; the ARPAbet
#: symbols follow and are only reachable through {curly brace} input)
SYMBOLS = ['_'] + list('-') + list('!\'(),.:;? ') + list('ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz')
_ID = {s: i for i, s in enumerate(SYMBOLS)}


def text_to_ids(text):
    """`text_to_sequence(text, ['basic_cleaners'])` (utils/text/__init__.py:16-43, cleaners.py:69-73) for plain text: lowercase,
    collapse whitespace, drop unknown symbols and the pad.  The reference's default `english_cleaners` additionally
    transliterates and spells out numbers / abbreviations (needs unidecode + inflect); for text without those both agree."""
    text = re.sub(r'\s+', ' ', text.lower())
    return [_ID[c] for c in text if c in _ID and c not in '_~']


#: A form of the batched decoder kernel as `TacotronInference._decode_launch` drives it: the call struct, the plain and the groups entry point, the
#: workspace attributes of the first and the second group of a launch, the form's word in an error message; the per-sentence int32 table
#: (`count`, its values `counts(mels, S, steps, r)`) and the step limits that follow from it (`limits(counts, r)`); the table of ground-truth mels
#: (or None); whether a sentence ends on a stop test (`steps_done`, `stop_threshold`); `workspace(L, S, table, r)` -> (bytes a call needs, None or
#: a function for the bytes a NEW workspace gets if that is more); the ValueError text for a table the size function refuses (or None).
_DecodeForm = collections.namedtuple('_DecodeForm', 'struct plain grouped ws_names word count counts limits mel_table stop_test refused workspace')


class TacotronInference:
    def __init__(self, state_dict, device=None):
        dev = torch.device(device) if device is not None else None
        self.p = {k: (v.detach().to(dev) if dev is not None else v.detach()) for k, v in state_dict.items() if torch.is_tensor(v)}
        p = self.p
        self.device = p['encoder.embedding.weight'].device
        self.n_mels = p['decoder.prenet.fc1.weight'].shape[1]
        self.decoder_dims = p['decoder.attn_rnn.weight_hh'].shape[1]
        self.lstm_dims = p['decoder.res_rnn1.weight_hh'].shape[1]
        self.max_r = p['decoder.mel_proj.weight'].shape[0] // self.n_mels
        self.r = int(p['decoder.r'].item()) if 'decoder.r' in p else int(p.get('r', torch.tensor(1)).item())
        self.stop_threshold = float(p['stop_threshold'].item()) if 'stop_threshold' in p else -3.4
        self._enc_k = self._count('encoder.cbhg.conv1d_bank.%d.conv.weight')
        self._post_k = self._count('postnet.conv1d_bank.%d.conv.weight')
        self.last_front_path = None                # 'hip' / 'torch': what the last generate() ran the encoder and the post-net on
        self._front = None                         # wrnn_taco_front handle (one per instance), False: create refused the dims
        self._front_ws = None                      # its workspace, reused and grown
        self._dec_w = None                         # generate_batch: (wrnn_taco_weights, the tensors it points to), built once
        self._batch_ws = None                      # ... and the workspace of wrnn_taco_decode_batch, reused and grown
        self._forced_ws = None                     # forward_gta: the workspace of wrnn_taco_decode_forced, reused and grown
        self._batch_ws2 = self._forced_ws2 = None  # groups=2: the second group's workspaces of a grouped launch
        self.last_decode_groups = []               # generate_batch / forward_gta_batch: per native decode call, the sizes of the groups it decoded

    def _count(self, pattern):
        n = 0
        while pattern % n in self.p:
            n += 1
        return n

    # -- building blocks (eval mode) ----------------------------------------------------------------------------------
    def _bnconv(self, x, prefix, relu=True):
        """BatchNormConv (models/tacotron.py:43-54): conv (same padding) -> [relu] -> batch norm (running statistics)."""
        w = self.p[prefix + '.conv.weight']
        x = F.conv1d(x, w, None, 1, w.shape[2] // 2)
        if relu:
            x = F.relu(x)
        q = prefix + '.bnorm.'
        return F.batch_norm(x, self.p[q + 'running_mean'], self.p[q + 'running_var'], self.p[q + 'weight'], self.p[q + 'bias'], False, 0.0, 1e-5)

    def _prenet(self, x, prefix):
        """PreNet (:141-155) in eval mode: two linear + relu layers, dropout off."""
        x = F.relu(F.linear(x, self.p[prefix + '.fc1.weight'], self.p[prefix + '.fc1.bias']))
        return F.relu(F.linear(x, self.p[prefix + '.fc2.weight'], self.p[prefix + '.fc2.bias']))

    def _cbhg_front(self, x, prefix, K):
        """CBHG (:57-139) in front of its GRU: conv bank 1..K -> max pool -> two projections -> residual -> highways.  (1, n, channels)."""
        p = self.p
        n = x.size(-1)
        res = x
        bank = torch.cat([self._bnconv(x, f'{prefix}.conv1d_bank.{k}')[:, :, :n] for k in range(K)], dim=1)
        x = F.max_pool1d(bank, 2, 1, 1)[:, :, :n]
        x = self._bnconv(x, prefix + '.conv_project1')
        x = self._bnconv(x, prefix + '.conv_project2', relu=False)
        x = (x + res).transpose(1, 2)
        if prefix + '.pre_highway.weight' in p:
            x = F.linear(x, p[prefix + '.pre_highway.weight'])
        h = 0
        while f'{prefix}.highways.{h}.W1.weight' in p:
            q = f'{prefix}.highways.{h}.'
            x1 = F.linear(x, p[q + 'W1.weight'], p[q + 'W1.bias'])
            g = torch.sigmoid(F.linear(x, p[q + 'W2.weight'], p[q + 'W2.bias']))
            x = g * F.relu(x1) + (1. - g) * x
            h += 1
        return x

    def _cbhg(self, x, prefix, K):
        """CBHG (:57-139): `_cbhg_front` -> bidirectional GRU."""
        p = self.p
        x = self._cbhg_front(x, prefix, K)
        q = prefix + '.rnn.'
        flat = [p[q + n_] for n_ in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0', 'weight_ih_l0_reverse',
                                     'weight_hh_l0_reverse', 'bias_ih_l0_reverse', 'bias_hh_l0_reverse')]
        if getattr(self, '_bigru_kernel', False) and x.is_cuda and x.size(0) == 1 and flat[1].shape[1] == 128:
            return self._bigru(x, flat)
        hx = torch.zeros(2, x.size(0), flat[1].shape[1], device=x.device, dtype=x.dtype)
        out, _ = torch._VF.gru(x, hx, flat, True, 1, 0.0, False, True, True)
        return out

    def _bigru(self, x, flat):
        """The CBHG's bidirectional GRU (:95, :137) through `wrnn_bigru` (csrc/wrnn_taco.hip: one persistent workgroup per
        direction, W_hh in registers) instead of MIOpen's per-step launches; the input products are two plain GEMMs."""
        import ctypes
        from . import _lib
        L = _lib.lib()
        w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r = [t.contiguous() for t in flat]
        gi_f = F.linear(x[0], w_ih, b_ih).contiguous()
        gi_r = F.linear(x[0], w_ih_r, b_ih_r).contiguous()
        out = torch.empty(1, x.size(1), 256, device=x.device, dtype=torch.float32)
        c = _lib.BigruCall()
        c.struct_bytes = ctypes.sizeof(_lib.BigruCall)
        c.T, c.hidden = x.size(1), 128
        c.gi_fwd, c.gi_rev, c.w_hh_fwd, c.w_hh_rev = gi_f.data_ptr(), gi_r.data_ptr(), w_hh.data_ptr(), w_hh_r.data_ptr()
        c.b_hh_fwd, c.b_hh_rev, c.out = b_hh.data_ptr(), b_hh_r.data_ptr(), out.data_ptr()
        c.stream = torch.cuda.current_stream(x.device).cuda_stream
        rc = L.wrnn_bigru((x.device.index if x.device.index is not None else torch.cuda.current_device()), ctypes.byref(c))
        if rc != _lib.WRNN_OK:
            raise _lib.WrnnError(f'wrnn_bigru failed (rc={rc}): {L.wrnn_taco_last_error().decode()}')
        return out

    # -- the encoder and the post-net through the C ABI (csrc/wrnn_cbhg.hip) ---------------------------------------------
    def _cbhg_weights(self, c, prefix, K, keep):
        """Fill one `wrnn_cbhg_weights` from the state dict; False if it has more highways than the struct holds."""
        p = self.p

        def ptr(name):
            t = p[prefix + name].detach().to(self.device, torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()
        bank0 = p[prefix + 'conv1d_bank.0.conv.weight']
        c.K, c.in_channels, c.channels = K, bank0.shape[1], bank0.shape[0]
        c.proj1_channels, c.proj2_channels = p[prefix + 'conv_project1.conv.weight'].shape[0], p[prefix + 'conv_project2.conv.weight'].shape[0]
        for k in range(K):
            q = f'conv1d_bank.{k}.'
            c.bank_conv_w[k] = ptr(q + 'conv.weight')
            c.bank_bn_w[k], c.bank_bn_b[k] = ptr(q + 'bnorm.weight'), ptr(q + 'bnorm.bias')
            c.bank_bn_mean[k], c.bank_bn_var[k] = ptr(q + 'bnorm.running_mean'), ptr(q + 'bnorm.running_var')
        for i in (1, 2):
            q = f'conv_project{i}.'
            setattr(c, f'proj{i}_conv_w', ptr(q + 'conv.weight'))
            for a, b in (('w', 'weight'), ('b', 'bias'), ('mean', 'running_mean'), ('var', 'running_var')):
                setattr(c, f'proj{i}_bn_{a}', ptr(q + 'bnorm.' + b))
        if prefix + 'pre_highway.weight' in p:
            c.pre_highway_w = ptr('pre_highway.weight')
        h = self._count(prefix + 'highways.%d.W1.weight')
        if h > 4:
            return False
        c.num_highways = h
        for i in range(h):
            q = f'highways.{i}.'
            c.highway_w1[i], c.highway_b1[i] = ptr(q + 'W1.weight'), ptr(q + 'W1.bias')
            c.highway_w2[i], c.highway_b2[i] = ptr(q + 'W2.weight'), ptr(q + 'W2.bias')
        for a, b in (('rnn_w_ih', 'weight_ih_l0'), ('rnn_w_hh', 'weight_hh_l0'), ('rnn_b_ih', 'bias_ih_l0'), ('rnn_b_hh', 'bias_hh_l0')):
            setattr(c, a, ptr('rnn.' + b))
            setattr(c, a + '_rev', ptr('rnn.' + b + '_reverse'))
        return p[prefix + 'rnn.weight_hh_l0'].shape == (3 * c.channels, c.channels) and p[prefix + 'rnn.weight_ih_l0'].shape == (3 * c.channels, c.channels)

    def _front_handle(self):
        """The instance's `wrnn_taco_front` (created on first use), or None when `wrnn_taco_front_create` refuses the dims
        (WRNN_ERR_ARG: the caller stays on the torch ops).  Any other failure raises."""
        import ctypes
        from . import _lib
        if self._front is not None:
            return self._front or None
        if self.device.type != 'cuda':
            raise _lib.WrnnError('the encoder / post-net kernels need a HIP device (no CPU fallback)')
        L = _lib.lib()
        p, keep = self.p, []
        w = _lib.TacoFrontWeights()
        w.struct_bytes = ctypes.sizeof(_lib.TacoFrontWeights)
        w.n_symbols, w.embed_dims = p['encoder.embedding.weight'].shape
        w.prenet1, w.prenet2 = p['encoder.pre_net.fc1.weight'].shape[0], p['encoder.pre_net.fc2.weight'].shape[0]
        w.encoder_proj_dims, w.n_mels, w.fft_bins = p['encoder_proj.weight'].shape[0], self.n_mels, p['post_proj.weight'].shape[0]
        for a, b in (('embedding', 'encoder.embedding.weight'), ('prenet_fc1_w', 'encoder.pre_net.fc1.weight'), ('prenet_fc1_b', 'encoder.pre_net.fc1.bias'),
                     ('prenet_fc2_w', 'encoder.pre_net.fc2.weight'), ('prenet_fc2_b', 'encoder.pre_net.fc2.bias'), ('encoder_proj_w', 'encoder_proj.weight'),
                     ('post_proj_w', 'post_proj.weight')):
            t = p[b].detach().to(self.device, torch.float32).contiguous()
            keep.append(t)
            setattr(w, a, t.data_ptr())
        ok = self._cbhg_weights(w.encoder_cbhg, 'encoder.cbhg.', self._enc_k, keep) if 1 <= self._enc_k <= 16 else False
        ok = ok and (self._cbhg_weights(w.postnet, 'postnet.', self._post_k, keep) if 1 <= self._post_k <= 16 else False)
        ok = ok and p['encoder_proj.weight'].shape[1] == 2 * w.encoder_cbhg.channels and p['post_proj.weight'].shape[1] == 2 * w.postnet.channels
        if not ok:
            self._front = False
            return None
        torch.cuda.synchronize(self.device)                                        # the tensors above may be fresh copies: create reads them
        h = ctypes.c_void_p()
        self._front_device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        rc = L.wrnn_taco_front_create(ctypes.byref(w), self._front_device, ctypes.byref(h))
        if rc == _lib.ERR_ARG:
            self._front = False
            self._front_refused = L.wrnn_taco_last_error().decode()
            return None
        if rc != _lib.WRNN_OK:
            raise _lib.WrnnError(f'wrnn_taco_front_create failed (rc={rc}): {L.wrnn_taco_last_error().decode()}')
        self._front = h
        self._front_destroy = L.wrnn_taco_front_destroy
        return h

    def __del__(self):
        try:
            h = getattr(self, '_front', None)
            if h:
                self._front = None
                self._front_destroy(h)
        except Exception:
            pass

    def _grow(self, name, need, first=None):
        """The workspace kept as attribute `name` (uint8, on the device).  Where it is missing or shorter than `need` bytes it is replaced: by one
        of `need` bytes, or of `first()` if that is more."""
        if getattr(self, name) is None or getattr(self, name).numel() < need:
            setattr(self, name, torch.empty(max(need, first() if first else 0), dtype=torch.uint8, device=self.device))
        return getattr(self, name)

    def _front_lib(self):
        """(the library, the front handle) for an encoder / post-net kernel call; WrnnError where there is no handle."""
        from . import _lib
        L, h = _lib.lib(), self._front_handle()
        if h is None:
            raise _lib.WrnnError(f'wrnn_taco_front_create refused these dims: {getattr(self, "_front_refused", "unsupported state dict")}')
        return L, h

    def _front_workspace(self, L, h, lengths, many):
        """(the front workspace, grown for a call over sentences of `lengths` rows; the call's count arguments: (rows,), or `many`: (the HOST
        table of the lengths, their number)).  ValueError for a table the library refuses, before anything is uploaded or allocated."""
        import ctypes
        from . import _lib
        if not many:
            return self._grow('_front_ws', int(L.wrnn_taco_front_workspace_bytes(h, lengths[0]))), (lengths[0],)
        n = (ctypes.c_int32 * len(lengths))(*lengths)
        need = int(L.wrnn_taco_front_workspace_bytes_many(h, n, len(lengths)))
        if need == 0:
            raise ValueError(f'{len(lengths)} sentences of lengths {list(lengths)}: 1..{_lib.TACO_FRONT_MANY_MAX} sentences of 1..2^20 rows per call')
        return self._grow('_front_ws', need), (n, len(lengths))

    def _front_call(self, L, h, entry, source, count, ws, lengths, *, widths, pre_width):
        """`entry(h, source, *count, outputs, workspace, stream)`: one encoder / post-net call over sentences of `lengths` rows.  The outputs are
        allocated here, (rows, width) each: one per entry of `widths`, then the highway output in front of the GRU (`pre_width`; None: not
        wanted, and None in the result).  Returns per sentence the tuple of its rows of every output.  Asynchronous on the current stream."""
        from . import _lib
        rows = sum(lengths)
        outs = [torch.empty(rows, w, device=self.device) for w in widths] + [torch.empty(rows, pre_width, device=self.device) if pre_width else None]
        rc = getattr(L, entry)(h, source, *count, *[t.data_ptr() if t is not None else None for t in outs], ws.data_ptr(), ws.numel(),
                               torch.cuda.current_stream(self.device).cuda_stream)
        if rc != _lib.WRNN_OK:
            raise _lib.WrnnError(f'{entry} failed (rc={rc}): {L.wrnn_taco_last_error().decode()}')
        if len(lengths) == 1:
            return [tuple(outs)]
        ends = np.cumsum(lengths)
        return [tuple(t[e - k:e] if t is not None else None for t in outs) for k, e in zip(lengths, ends.tolist())]

    def _encode_run(self, ids, lengths, want_pre_rnn):
        """`encode_kernel` (lengths None: `ids` is one sentence) / `encode_kernel_many` (`ids`: the sentences of `lengths` ids, concatenated)."""
        L, h = self._front_lib()
        many = lengths is not None
        ids_h = torch.as_tensor(ids, dtype=torch.int32, device='cpu').contiguous()
        lengths = lengths if many else [ids_h.numel()]
        ws, count = self._front_workspace(L, h, lengths, many)                     # (a refused table: before the upload)
        ids_d = ids_h.to(self.device)
        D, C2 = self.p['encoder_proj.weight'].shape
        rows = self._front_call(L, h, 'wrnn_taco_encode_many' if many else 'wrnn_taco_encode', ids_d.data_ptr(), count, ws, lengths,
                                widths=(C2, D), pre_width=C2 // 2 if want_pre_rnn else None)
        return [(seq.unsqueeze(0), seq_proj.unsqueeze(0), pre) for seq, seq_proj, pre in rows]

    def encode_kernel(self, ids, want_pre_rnn=False):
        """`encode` through `wrnn_taco_encode`: (encoder_seq (1, n, 2C), its projection (1, n, D), the highway output (n, C) in front of the
        GRU or None).  Asynchronous on the current stream."""
        return self._encode_run(ids, None, want_pre_rnn)[0]

    def encode_kernel_many(self, list_of_ids, want_pre_rnn=False):
        """`encode_kernel` for a list of 1..64 sentences through ONE `wrnn_taco_encode_many` call (one host-to-device copy of the concatenated
        ids, every stage one launch for all sentences).  Returns per sentence (encoder_seq (1, n, 2C), its projection (1, n, D), the highway
        output (n, C) or None): views of the call's concatenated outputs, each bit-identical to `encode_kernel` of that sentence alone.
        Asynchronous on the current stream."""
        return self._encode_run([int(i) for ids in list_of_ids for i in ids], [len(ids) for ids in list_of_ids], want_pre_rnn)

    def _postnet_run(self, list_of_mels, many, want_pre_rnn):
        import ctypes
        L, h = self._front_lib()
        ms = [mel.reshape(self.n_mels, -1).to(self.device, torch.float32).contiguous() for mel in list_of_mels]
        lengths = [m.size(1) for m in ms]
        ws, count = self._front_workspace(L, h, lengths, many)
        source = (ctypes.c_void_p * len(ms))(*[m.data_ptr() for m in ms]) if many else ms[0].data_ptr()
        fft, C2 = self.p['post_proj.weight'].shape
        return self._front_call(L, h, 'wrnn_taco_postnet_many' if many else 'wrnn_taco_postnet', source, count, ws, lengths,
                                widths=(fft,), pre_width=C2 // 2 if want_pre_rnn else None)

    def postnet_kernel(self, mel, want_pre_rnn=False):
        """The post-net CBHG and `post_proj` through `wrnn_taco_postnet`: mel (1, n_mels, N) or (n_mels, N) on the device -> (linear (N, fft),
        the highway output (N, C) or None).  Asynchronous on the current stream."""
        return self._postnet_run([mel], False, want_pre_rnn)[0]

    def postnet_kernel_many(self, list_of_mels, want_pre_rnn=False):
        """`postnet_kernel` for a list of 1..64 mels ((1, n_mels, N_s) or (n_mels, N_s) each) through ONE `wrnn_taco_postnet_many` call.  Returns per
        sentence (linear (N_s, fft), the highway output (N_s, C) or None): views of the call's concatenated outputs, each bit-identical to
        `postnet_kernel` of that mel alone.  Asynchronous on the current stream."""
        return self._postnet_run(list_of_mels, True, want_pre_rnn)

    def encode(self, ids):
        """Encoder (:24-39) + `encoder_proj` (:403-404): ids (n,) -> encoder_seq (1, n, 2C), its projection (1, n, D)."""
        x = torch.as_tensor(ids, dtype=torch.long, device=self.device).unsqueeze(0)
        x = F.embedding(x, self.p['encoder.embedding.weight'])
        x = self._prenet(x, 'encoder.pre_net').transpose(1, 2)
        seq = self._cbhg(x, 'encoder.cbhg', self._enc_k)
        return seq, F.linear(seq, self.p['encoder_proj.weight'])

    def _decoder_step(self, seq, seq_proj, prenet_in, st):
        """Decoder.forward (:218-279) in eval mode with the LSA attention (:181-207); `st` holds the recurrent tensors and is
        updated IN PLACE."""
        p = self.p
        q = 'decoder.'
        pre = self._prenet(prenet_in, q + 'prenet')
        attn_h = torch.gru_cell(torch.cat([st['context'], pre], dim=-1), st['attn_h'], p[q + 'attn_rnn.weight_ih'], p[q + 'attn_rnn.weight_hh'],
                                p[q + 'attn_rnn.bias_ih'], p[q + 'attn_rnn.bias_hh'])
        # location-sensitive attention with sigmoid-normalised ("smooth") scores
        pq = F.linear(attn_h, p[q + 'attn_net.W.weight'], p[q + 'attn_net.W.bias']).unsqueeze(1)
        loc = torch.cat([st['cumulative'].unsqueeze(1), st['attention'].unsqueeze(1)], dim=1)
        kw = p[q + 'attn_net.conv.weight']
        ploc = F.linear(F.conv1d(loc, kw, None, 1, (kw.shape[2] - 1) // 2).transpose(1, 2), p[q + 'attn_net.L.weight'], p[q + 'attn_net.L.bias'])
        u = F.linear(torch.tanh(pq + seq_proj + ploc), p[q + 'attn_net.v.weight']).squeeze(-1)
        scores = torch.sigmoid(u) / torch.sigmoid(u).sum(dim=1, keepdim=True)
        st['attention'].copy_(scores)
        st['cumulative'].add_(scores)
        context = (scores.unsqueeze(-1).transpose(1, 2) @ seq).squeeze(1)
        x = F.linear(torch.cat([context, attn_h], dim=1), p[q + 'rnn_input.weight'], p[q + 'rnn_input.bias'])
        h1, c1 = torch.lstm_cell(x, (st['h1'], st['c1']), p[q + 'res_rnn1.weight_ih'], p[q + 'res_rnn1.weight_hh'], p[q + 'res_rnn1.bias_ih'],
                                 p[q + 'res_rnn1.bias_hh'])
        x = x + h1
        h2, c2 = torch.lstm_cell(x, (st['h2'], st['c2']), p[q + 'res_rnn2.weight_ih'], p[q + 'res_rnn2.weight_hh'], p[q + 'res_rnn2.bias_ih'],
                                 p[q + 'res_rnn2.bias_hh'])
        x = x + h2
        mels = F.linear(x, p[q + 'mel_proj.weight']).view(x.size(0), self.n_mels, self.max_r)[:, :, :self.r]
        for k, v in (('attn_h', attn_h), ('context', context), ('h1', h1), ('c1', c1), ('h2', h2), ('c2', c2)):
            st[k].copy_(v)
        return mels, scores

    def _decode_kernel(self, seq, seq_proj, steps, variant=0):
        """The decoder loop (:396-414) as ONE persistent HIP kernel (csrc/wrnn_taco.hip) through the C ABI
        (`wrnn_taco_decode`; variant 0 = auto, 1 = the flag-barrier kernel, 2 = the register-resident kernel).  Returns (mel (1, n_mels, N) , attention (N / r, n)) device tensors; fails loudly without the
        extension or a HIP device -- there is no host fallback."""
        import ctypes
        from . import _lib
        dev = self.device
        if dev.type != 'cuda':
            raise _lib.WrnnError('the Tacotron decoder kernel needs a HIP device (no CPU fallback)')
        L = _lib.lib()
        n = seq.size(1)
        max_steps = (steps + self.r - 1) // self.r
        seq_c, proj_c = seq[0].contiguous(), seq_proj[0].contiguous()
        mel_out = torch.zeros(max_steps, self.n_mels, self.r, device=dev)
        scores = torch.zeros(max_steps, n, device=dev)
        done = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(int(L.wrnn_taco_workspace_bytes()), dtype=torch.uint8, device=dev)
        c = _lib.TacoCall()
        c.struct_bytes = ctypes.sizeof(_lib.TacoCall)
        c.n, c.r, c.max_r, c.max_steps, c.stop_threshold = n, self.r, self.max_r, max_steps, self.stop_threshold
        c.seq, c.seq_proj, c.mel_out, c.scores_out = seq_c.data_ptr(), proj_c.data_ptr(), mel_out.data_ptr(), scores.data_ptr()
        c.steps_done, c.workspace, c.workspace_bytes = done.data_ptr(), ws.data_ptr(), ws.numel()
        c.stream = torch.cuda.current_stream(dev).cuda_stream
        c.variant = int(variant)
        rc = L.wrnn_taco_decode((dev.index if dev.index is not None else torch.cuda.current_device()), ctypes.byref(self.decoder_weights()), ctypes.byref(c))
        if rc != _lib.WRNN_OK:
            raise _lib.WrnnError(f'wrnn_taco_decode failed (rc={rc}): {L.wrnn_taco_last_error().decode()}')
        st4 = (ctypes.c_uint32 * 4)()
        rc = L.wrnn_taco_status(ws.data_ptr(), ctypes.byref(st4), c.stream)
        if rc != _lib.WRNN_OK or st4[0] != 0:
            raise _lib.WrnnError(f'Tacotron decoder kernel failed: status {list(st4)} {L.wrnn_taco_last_error().decode()}')
        self._last_taco_ws = ws                                                    # (variant 3: the profile words are its last 192 bytes)
        k = int(done.item())
        mel = mel_out[:k].permute(1, 0, 2).reshape(1, self.n_mels, k * self.r)      # frames of step s at columns [s r, (s+1) r)
        return mel, scores[:k]

    _DEC_NAMES = dict(prenet_fc1_w='prenet.fc1.weight', prenet_fc1_b='prenet.fc1.bias', prenet_fc2_w='prenet.fc2.weight',
                      prenet_fc2_b='prenet.fc2.bias', attn_rnn_w_ih='attn_rnn.weight_ih', attn_rnn_w_hh='attn_rnn.weight_hh',
                      attn_rnn_b_ih='attn_rnn.bias_ih', attn_rnn_b_hh='attn_rnn.bias_hh', attn_W_w='attn_net.W.weight',
                      attn_W_b='attn_net.W.bias', attn_conv_w='attn_net.conv.weight', attn_L_w='attn_net.L.weight',
                      attn_L_b='attn_net.L.bias', attn_v_w='attn_net.v.weight', rnn_input_w='rnn_input.weight',
                      rnn_input_b='rnn_input.bias', rnn1_w_ih='res_rnn1.weight_ih', rnn1_w_hh='res_rnn1.weight_hh',
                      rnn1_b_ih='res_rnn1.bias_ih', rnn1_b_hh='res_rnn1.bias_hh', rnn2_w_ih='res_rnn2.weight_ih',
                      rnn2_w_hh='res_rnn2.weight_hh', rnn2_b_ih='res_rnn2.bias_ih', rnn2_b_hh='res_rnn2.bias_hh',
                      mel_proj_w='mel_proj.weight')

    def decoder_weights(self):
        """This instance's `wrnn_taco_weights` (the decoder's tensors as float32 device pointers), built on first use and kept: the struct and
        the tensors it points to live as long as the instance."""
        import ctypes
        from . import _lib
        if self._dec_w is None:
            keep = {k: self.p['decoder.' + v].detach().to(self.device, torch.float32).contiguous() for k, v in self._DEC_NAMES.items()}
            w = _lib.TacoWeights()
            w.struct_bytes = ctypes.sizeof(_lib.TacoWeights)
            w.n_mels, w.prenet1, w.prenet2 = self.n_mels, keep['prenet_fc1_w'].shape[0], keep['prenet_fc2_w'].shape[0]
            w.decoder_dims, w.encoder_width, w.lstm_dims = self.decoder_dims, self.p['encoder_proj.weight'].shape[1], self.lstm_dims
            w.attn_filters, w.attn_kernel = keep['attn_conv_w'].shape[0], keep['attn_conv_w'].shape[2]
            for k, tns in keep.items():
                setattr(w, k, tns.data_ptr())
            self._dec_w = (w, keep)
        return self._dec_w[0]

    # The two forms of the batched decoder kernel as `_decode_launch` drives them (`_DecodeForm`, above).
    _FREE = _DecodeForm(
        struct='TacoBatchCall', plain='wrnn_taco_decode_batch', grouped='wrnn_taco_decode_batch_groups', ws_names=('_batch_ws', '_batch_ws2'),
        word='batched', count='max_steps', counts=lambda mels, S, steps, r: [(steps + r - 1) // r] * S, limits=lambda counts, r: counts,
        mel_table=None, stop_test=True, refused=None,
        # (a new workspace holds at least the full batch of that many sentences)
        workspace=lambda L, S, table, r: (L.wrnn_taco_batch_workspace_bytes(S), lambda: int(L.wrnn_taco_batch_workspace_bytes(min(TACO_BATCH_MAX, max(S, 1))))))
    _FORCED = _DecodeForm(
        struct='TacoForcedCall', plain='wrnn_taco_decode_forced', grouped='wrnn_taco_decode_forced_groups', ws_names=('_forced_ws', '_forced_ws2'),
        word='forced', count='frames', counts=lambda mels, S, steps, r: [m.size(1) for m in mels],
        limits=lambda counts, r: [(k + r - 1) // r for k in counts], mel_table='force_mel', stop_test=False,
        refused='{S} sentences of {counts} frames at r={r}: 1..%d sentences of 1..2^20 frames per call' % TACO_BATCH_MAX,
        workspace=lambda L, S, table, r: (L.wrnn_taco_forced_workspace_bytes(S, table, r), None))

    def _decode_launch(self, form, groups, steps=None):
        """The decoder loops of ONE or TWO groups of sentences in the form `form`.  A group is (encs, mels): encs as `_decode_batch_kernel` takes
        them; mels the ground-truth mels of `_FORCED` (a sentence runs ceil(frames / r) steps), None for `_FREE` (every sentence runs at most
        ceil(steps / r) steps and ends on its own stop test).  One group: the plain entry point.  Two: ONE launch of the groups entry point, a
        group on each half of a 256-CU device, every group with a workspace of its own (for `_FORCED`, a pre-pass per group in front); where
        the device refuses the 256 co-resident workgroups (WRNN_ERR_RESIDENCY, nothing written) the groups take the plain call one after the
        other.  Returns the groups' results in order; `last_decode_groups` gains one entry per native call."""
        import ctypes
        from . import _lib
        dev, r = self.device, self.r
        if dev.type != 'cuda':
            raise _lib.WrnnError('the Tacotron decoder kernel needs a HIP device (no CPU fallback)')
        if not 1 <= len(groups) <= _lib.TACO_GROUPS_MAX:
            raise ValueError(f'{len(groups)} groups: a launch decodes 1..{_lib.TACO_GROUPS_MAX}')
        L, plain, grouped, word = _lib.lib(), form.plain, form.grouped, form.word
        device = dev.index if dev.index is not None else torch.cuda.current_device()
        calls = []
        for ws_name, (encs, mels) in zip(form.ws_names, groups):
            S = len(encs)
            seqs = [e[0][0].to(torch.float32).contiguous() for e in encs]
            projs = [e[1][0].to(torch.float32).contiguous() for e in encs]
            mels = [m.contiguous() for m in mels] if form.mel_table else None
            counts = form.counts(mels, S, steps, r)
            limits = form.limits(counts, r)
            table = (ctypes.c_int32 * S)(*counts)
            need, first = form.workspace(L, S, table, r)
            if need == 0 and form.refused:
                raise ValueError(form.refused.format(S=S, counts=counts, r=r))
            ws = self._grow(ws_name, int(need), first)
            outs = [torch.zeros(k, self.n_mels, r, device=dev) for k in limits]
            scores = [torch.zeros(k, q.size(0), device=dev) for k, q in zip(limits, seqs)]
            done = torch.zeros(S, dtype=torch.int32, device=dev) if form.stop_test else None   # (None: a sentence runs all its steps)
            c = getattr(_lib, form.struct)()
            c.struct_bytes = ctypes.sizeof(c)
            c.n_sent, c.r, c.max_r = S, r, self.max_r
            c.n = (ctypes.c_int32 * S)(*[q.size(0) for q in seqs])
            setattr(c, form.count, table)
            if form.stop_test:
                c.steps_done, c.stop_threshold = done.data_ptr(), self.stop_threshold
            for field, ts in ((form.mel_table, mels), ('seq', seqs), ('seq_proj', projs), ('mel_out', outs), ('scores_out', scores)):
                if field:
                    setattr(c, field, (ctypes.c_void_p * S)(*[t.data_ptr() for t in ts]))
            c.workspace, c.workspace_bytes = ws.data_ptr(), ws.numel()
            c.stream = torch.cuda.current_stream(dev).cuda_stream
            calls.append((c, ws, outs, scores, limits, done, (seqs, projs, mels)))

        def finish(call):
            c, ws, outs, scores, limits, done, _ = call
            st4 = (ctypes.c_uint32 * 4)()
            rc = L.wrnn_taco_status(ws.data_ptr(), ctypes.byref(st4), c.stream)
            if rc != _lib.WRNN_OK or st4[0] != 0:
                raise _lib.WrnnError(f'Tacotron {word} decoder kernel failed: status {list(st4)} {L.wrnn_taco_last_error().decode()}')
            ks = limits if done is None else [int(k) for k in done.cpu()]
            return [(m[:k].permute(1, 0, 2).reshape(1, self.n_mels, k * r), a[:k]) for m, a, k in zip(outs, scores, ks)]

        if len(calls) == 2:
            table = (ctypes.POINTER(getattr(_lib, form.struct)) * 2)(*[ctypes.pointer(call[0]) for call in calls])
            rc = getattr(L, grouped)(device, ctypes.byref(self.decoder_weights()), table, 2)
            if rc == _lib.WRNN_OK:
                self.last_decode_groups.append(tuple(len(g[0]) for g in groups))
                return [finish(call) for call in calls]
            if rc != _lib.ERR_RESIDENCY:
                raise _lib.WrnnError(f'{grouped} failed (rc={rc}): {L.wrnn_taco_last_error().decode()}')
        out = []
        for call, g in zip(calls, groups):
            rc = getattr(L, plain)(device, ctypes.byref(self.decoder_weights()), ctypes.byref(call[0]))
            if rc != _lib.WRNN_OK:
                raise _lib.WrnnError(f'{plain} failed (rc={rc}): {L.wrnn_taco_last_error().decode()}')
            self.last_decode_groups.append((len(g[0]),))
            out.append(finish(call))
        return out

    def _decode_batch_kernel(self, encs, steps):
        """The decoder loops of up to `_lib.TACO_BATCH_MAX` sentences in ONE persistent kernel (`wrnn_taco_decode_batch`,
        csrc/wrnn_taco_batch.hip).  encs: [(seq (1, n, 256), seq_proj (1, n, 256))], every n <= `_lib.TACO_BATCH_NMAX`.  Returns
        [(mel (1, n_mels, N_s), attention (N_s / r, n_s))] device tensors, each bit-identical to `_decode_kernel(..., variant=2)`."""
        return self._decode_batch_launch([encs], steps)[0]

    def _decode_batch_launch(self, groups, steps):
        """`_decode_launch` for ONE or TWO groups of free-running sentences (each as `_decode_batch_kernel` takes them): `wrnn_taco_decode_batch`,
        or ONE `wrnn_taco_decode_batch_groups` launch."""
        return self._decode_launch(self._FREE, [(encs, None) for encs in groups], steps)

    @staticmethod
    def _pair_groups(groups, n):
        """The decoder groups of a pass as the launches that decode them: n = 1, one group per launch (the plain call); n = 2, consecutive groups in
        pairs (one grouped launch each), an odd group out alone.  The order of the groups is kept."""
        if isinstance(n, bool) or n not in (1, 2):
            raise ValueError(f'groups={n!r}: 1 (one group of sentences per launch) or 2 (two, on a device of 256 CUs)')
        return [groups[i:i + n] for i in range(0, len(groups), n)]

    # -- what generate / forward_gta and their batch forms share around the decoder -------------------------------------------------
    def _front_path(self, kernel, cbhg_kernel):
        """Where the encoder and the post-net run: True for `wrnn_taco_encode` / `wrnn_taco_postnet` (cbhg_kernel, and a state dict
        `wrnn_taco_front_create` takes), False for the torch ops -- with the CBHGs' GRUs as `wrnn_bigru` where `kernel` says so."""
        if cbhg_kernel and self.device.type != 'cuda':
            from . import _lib
            raise _lib.WrnnError('the encoder / post-net kernels need a HIP device (no CPU fallback)')
        self._bigru_kernel = bool(kernel) and self.device.type == 'cuda'           # the CBHGs' GRUs as persistent kernels too
        front = bool(cbhg_kernel) and self._front_handle() is not None
        self.last_front_path = 'hip' if front else 'torch'
        return front

    def _postnet(self, mel, front):
        """The post-net CBHG and `post_proj` (:416-421) over a decoded mel (1, n_mels, N): linear (fft, N), a device tensor."""
        if front:
            return self.postnet_kernel(mel)[0].transpose(0, 1)
        return F.linear(self._cbhg(mel, 'postnet', self._post_k), self.p['post_proj.weight']).transpose(1, 2)[0]

    def _check_batch(self, max_batch, groups):
        from . import _lib
        if not 1 <= int(max_batch) <= _lib.TACO_BATCH_MAX:
            raise ValueError(f'max_batch={max_batch}: 1..{_lib.TACO_BATCH_MAX}')
        self._pair_groups([], groups)                                              # (ValueError for anything but 1 or 2)

    def _batch_frame(self, list_of_ids, front, groups, form_groups, decode, decode_long):
        """`generate_batch` and `forward_gta_batch` behind their argument checks: encode all sentences, decode those of at most
        `_lib.TACO_BATCH_NMAX` ids in groups -- `form_groups(their indices)` forms the groups, `_pair_groups` the launches, and
        `decode(encs, launch)` returns the results of a launch's one or two groups -- and the others through `decode_long(i, enc)`, then run the
        post-net.  Returns per sentence numpy (mel, linear, attention)."""
        from . import _lib
        M = _lib.TACO_FRONT_MANY_MAX
        if front:
            # all sentences side by side, <= 64 per call; a call of ONE sentence goes through the single-sentence entry point (the same bits; the
            # sentence table costs 1-2 % there: DESIGN.md section 6)
            enc_many = lambda chunk: self.encode_kernel_many(chunk) if len(chunk) > 1 else [self.encode_kernel(chunk[0])]
            post_many = lambda chunk: self.postnet_kernel_many(chunk) if len(chunk) > 1 else [self.postnet_kernel(chunk[0])]
            encs = [e[:2] for c in range(0, len(list_of_ids), M) for e in enc_many(list_of_ids[c:c + M])]
        else:
            encs = [self.encode(ids) for ids in list_of_ids]
        decoded = [None] * len(encs)
        self.last_decode_groups = []
        for launch in self._pair_groups(form_groups([i for i, e in enumerate(encs) if e[0].size(1) <= _lib.TACO_BATCH_NMAX]), groups):
            for group, result in zip(launch, decode(encs, launch)):
                for i, d in zip(group, result):
                    decoded[i] = d
        for i, e in enumerate(encs):
            if decoded[i] is None:
                decoded[i] = decode_long(i, e)
        out = []
        if not front:
            for mel, attn in decoded:
                linear = self._postnet(mel, False)
                out.append((mel[0].cpu().numpy(), linear.cpu().numpy(), attn.cpu().numpy()))
            return out
        # one post-net pass over all decoded mels (<= 64 per call), then ONE transfer: every result flattened into one device buffer
        mels = [d[0] for d in decoded]
        lins = [l for c in range(0, len(mels), M) for l, _ in post_many(mels[c:c + M])]
        parts = [t.reshape(-1) for (mel, attn), lin in zip(decoded, lins) for t in (mel[0], lin, attn)]
        flat, o = torch.cat(parts).cpu().numpy() if parts else None, 0
        for (mel, attn), lin in zip(decoded, lins):
            trio = []
            for t in (mel[0], lin, attn):
                trio.append(flat[o:o + t.numel()].reshape(tuple(t.shape)))
                o += t.numel()
            out.append((trio[0], trio[1].T, trio[2]))                              # linear (fft, N), as `generate()` returns it
        return out

    @torch.no_grad()
    def generate_batch(self, list_of_ids, steps=2000, kernel=True, cbhg_kernel=False, max_batch=8, groups=1):
        """`generate()` for a list of sentences: a list of (mel, linear, attention), one per sentence, as `generate()` returns them.

        kernel=True (HIP device): the decoder loops run in groups of at most `max_batch` (1..8) sentences through `wrnn_taco_decode_batch` -- one
        persistent kernel per group, every sentence ending on its own stop test, each result bit-identical to the single-sentence kernel's.  A
        sentence of more than `_lib.TACO_BATCH_NMAX` ids goes through the single-sentence kernel.  cbhg_kernel=False: the encoder and the post-net
        run per sentence on the torch ops, as in `generate(kernel=True)`.  cbhg_kernel=True: ONE `wrnn_taco_encode_many` call encodes all
        sentences in front of the decoder groups and ONE `wrnn_taco_postnet_many` call runs the post-net over all decoded mels (64 sentences per
        call at most; a call of one sentence takes the single-sentence entry points), each sentence's bits those of `generate(kernel=True,
        cbhg_kernel=True)`; the results reach the host in one transfer at the end.  kernel=False: a loop of `generate()`, on any device.

        groups=2 (opt-in; a device of 256 CUs): consecutive decoder groups ride in pairs on ONE `wrnn_taco_decode_batch_groups` launch, a group on
        each half of the device -- 2 x `max_batch` sentences per launch, the same bits; an odd group out takes the plain call, and so do both
        groups of a pair where the device refuses the launch.  `last_decode_groups` lists what ran: per native call, its groups' sizes."""
        if not kernel:
            return [self.generate(ids, steps=steps, kernel=False, cbhg_kernel=cbhg_kernel) for ids in list_of_ids]
        self._check_batch(max_batch, groups)
        if self.device.type != 'cuda':
            from . import _lib
            raise _lib.WrnnError('the Tacotron decoder kernel needs a HIP device (no CPU fallback)')
        B = int(max_batch)

        def decode(encs, launch):
            g = [[encs[i] for i in group] for group in launch]
            return [self._decode_batch_kernel(g[0], steps)] if len(g) == 1 else self._decode_batch_launch(g, steps)
        return self._batch_frame(list_of_ids, self._front_path(True, cbhg_kernel), groups, lambda short: [short[g:g + B] for g in range(0, len(short), B)],
                                 decode, lambda i, e: self._decode_kernel(e[0], e[1], steps))

    # -- ground-truth-aligned mels: the teacher-forced decoder ------------------------------------------------------------------
    def _forced_mel(self, mel):
        """A ground-truth mel (n_mels, N) or (1, n_mels, N), numpy or tensor -> contiguous float32 (n_mels, N) on the device."""
        m = torch.as_tensor(np.asarray(mel) if not torch.is_tensor(mel) else mel).to(self.device, torch.float32)
        m = m.reshape(self.n_mels, -1).contiguous()
        if m.size(1) < 1:
            raise ValueError('a ground-truth mel needs at least one frame')
        return m

    def _decode_forced_eager(self, seq, seq_proj, m):
        """The teacher-forced loop of `Tacotron.forward(x, m, generate_gta=True)` (:347-354) over `_decoder_step`, on any device: decoder step k
        reads column k r - 1 of `m` (n_mels, N), the <GO> frame at k = 0; ceil(N / r) steps, no stop test.  Returns (mel (1, n_mels, steps r),
        attention (steps, n)) device tensors."""
        dev, n = self.device, seq.size(1)
        m = m.to(seq.dtype)
        z = lambda *s: torch.zeros(*s, device=dev, dtype=seq.dtype)            # (a float64 state dict decodes in float64)
        st = dict(attn_h=z(1, self.decoder_dims), h1=z(1, self.lstm_dims), h2=z(1, self.lstm_dims), c1=z(1, self.lstm_dims),
                  c2=z(1, self.lstm_dims), context=z(1, self.decoder_dims), cumulative=z(1, n), attention=z(1, n))
        frames, scores = [], []
        for t in range(0, m.size(1), self.r):
            prenet_in = m[:, t - 1].unsqueeze(0) if t > 0 else z(1, self.n_mels)
            m_, s_ = self._decoder_step(seq, seq_proj, prenet_in, st)
            frames.append(m_)
            scores.append(s_.clone())
        return torch.cat(frames, dim=2), torch.cat(scores, 0)

    def _decode_forced_kernel(self, encs, mels):
        """The teacher-forced decoder loops of up to `_lib.TACO_BATCH_MAX` sentences in ONE `wrnn_taco_decode_forced` call (the PreNet pre-pass
        and the forced form of the batched persistent kernel, csrc/wrnn_taco_batch.hip).  encs: [(seq (1, n, 256), seq_proj (1, n, 256))], every
        n <= `_lib.TACO_BATCH_NMAX`; mels: [(n_mels, N_s) float32 device tensors].  Returns [(mel (1, n_mels, steps_s r), attention (steps_s,
        n_s))] device tensors.  Fails loudly without the extension or a HIP device -- there is no host fallback."""
        return self._decode_forced_launch([(encs, mels)])[0]

    def _decode_forced_launch(self, groups):
        """`_decode_launch` for ONE or TWO teacher-forced groups, each an (encs, mels) pair as `_decode_forced_kernel` takes it:
        `wrnn_taco_decode_forced`, or ONE `wrnn_taco_decode_forced_groups` launch."""
        return self._decode_launch(self._FORCED, groups)

    @staticmethod
    def _gta_groups(steps, max_batch):
        """Groups of at most `max_batch` sentence indices, sentences sorted by their step count first (a stable sort), so that the sentences of
        one kernel end close to each other."""
        order = sorted(range(len(steps)), key=lambda i: steps[i])
        return [order[g:g + max_batch] for g in range(0, len(order), max_batch)]

    @torch.no_grad()
    def forward_gta(self, ids, mel, kernel=False, cbhg_kernel=False):
        """Ground-truth-aligned (GTA) features of one utterance: the reference's `Tacotron.forward(x, m, generate_gta=True)` (:310-368) at batch
        size 1 -- the decoder run TEACHER-FORCED over the recording's own mel `mel` (n_mels, N) on the decoder's scale ([-4, 4]): step k reads
        column k r - 1 of it (the <GO> frame at k = 0), steps = ceil(N / r), no stop test.  Returns numpy (gta (n_mels, steps r), linear (fft,
        steps r), attention (steps, n_chars)) -- the reference's three returns.

        kernel=False: the eager loop over `_decoder_step`, on any device.  kernel=True (HIP device): `wrnn_taco_decode_forced` -- a PreNet
        pre-pass over all steps and the forced form of the batched persistent kernel (csrc/wrnn_taco_batch.hip) -- for sentences of at most
        `_lib.TACO_BATCH_NMAX` ids; cbhg_kernel as in `generate()`.

        Two deliberate differences from the reference's `train_tacotron.py --force_gta`.  MODE: `create_gta_features` (:178-199) calls
        `model(x, mels)` WITHOUT generate_gta, so the checked-in script runs in train mode (PreNet dropout, batch statistics in the batch
        norms); this is the eval form the signature offers, the only deterministic one.  PADDING: the reference pads a batch's texts with zeros
        and attends over the padding, so an utterance's features depend on its batch companions; here every sentence is decoded as if alone
        (the reference at batch size 1)."""
        front = self._front_path(kernel, cbhg_kernel)
        m = self._forced_mel(mel)
        seq, seq_proj = self.encode_kernel(ids)[:2] if front else self.encode(ids)
        if kernel:
            from . import _lib
            if seq.size(1) > _lib.TACO_BATCH_NMAX:
                raise ValueError(f'{seq.size(1)} ids: the forced kernel takes sentences of at most {_lib.TACO_BATCH_NMAX} (kernel=False, or forward_gta_batch)')
            gta, attn = self._decode_forced_kernel([(seq, seq_proj)], [m])[0]
        else:
            gta, attn = self._decode_forced_eager(seq, seq_proj, m)
        linear = self._postnet(gta, front)
        return gta[0].cpu().numpy(), linear.cpu().numpy(), attn.cpu().numpy()

    @torch.no_grad()
    def forward_gta_batch(self, list_of_ids, list_of_mels, kernel=True, cbhg_kernel=False, max_batch=8, groups=1):
        """`forward_gta()` for a list of utterances: a list of (gta, linear, attention), one per utterance in the caller's order, as
        `forward_gta()` returns them (see there for the two deliberate differences from the reference's script: eval mode, and every sentence
        decoded as if alone -- the result does not depend on what rides along).

        kernel=True (HIP device): the sentences are sorted by their step count and decoded in groups of at most `max_batch` (1..8) through
        `wrnn_taco_decode_forced`, one persistent kernel per group, so a group's ragged ends waste little.  A sentence of more than
        `_lib.TACO_BATCH_NMAX` (256) ids goes through the EAGER loop on the device: there is no single-sentence forced kernel.
        cbhg_kernel=True: `encode_kernel_many` / `postnet_kernel_many` over all sentences (64 per call) and ONE transfer at the end, exactly as
        `generate_batch` does; otherwise the encoder and the post-net run per sentence on the torch ops.  kernel=False: a loop of
        `forward_gta(kernel=False)`, on any device.

        groups=2 (opt-in; a device of 256 CUs): consecutive groups of the sorted order ride in pairs on ONE `wrnn_taco_decode_forced_groups`
        launch, as in `generate_batch`; `last_decode_groups` lists what ran."""
        if len(list_of_ids) != len(list_of_mels):
            raise ValueError(f'{len(list_of_ids)} id lists for {len(list_of_mels)} mels')
        if not kernel:
            return [self.forward_gta(ids, mel, kernel=False, cbhg_kernel=cbhg_kernel) for ids, mel in zip(list_of_ids, list_of_mels)]
        self._check_batch(max_batch, groups)
        front = self._front_path(True, cbhg_kernel)
        ms = [self._forced_mel(mel) for mel in list_of_mels]

        def form_groups(short):                                                    # neighbours in the order of step counts: they end together
            steps = [(ms[i].size(1) + self.r - 1) // self.r for i in short]
            return [[short[j] for j in group] for group in self._gta_groups(steps, int(max_batch))]

        def decode(encs, launch):
            g = [([encs[i] for i in group], [ms[i] for i in group]) for group in launch]
            return [self._decode_forced_kernel(*g[0])] if len(g) == 1 else self._decode_forced_launch(g)
        # (more than 256 ids: the eager loop on the device)
        return self._batch_frame(list_of_ids, front, groups, form_groups, decode, lambda i, e: self._decode_forced_eager(e[0], e[1], ms[i]))

    @torch.no_grad()
    def generate(self, ids, steps=2000, kernel=False, kernel_variant=0, cbhg_kernel=False):
        """`Tacotron.generate(x, steps)` (:370-430).  Returns numpy (mel (n_mels, N), linear (fft, N), attention (N, n_chars)).

        kernel=True (HIP device): the decoder loop runs as ONE persistent kernel (`wrnn_taco_decode`, csrc/wrnn_taco.hip; the stop
        test of :411 is evaluated inside it) and the CBHGs' bidirectional GRUs as `wrnn_bigru`.  kernel=False: the eager loop (any
        device; the CPU form is the mirror tests/test_tacotron_mirror.py pins bit-exactly to the reference).  (Round 2's HIP-graph
        replay of one decoder step -- 555 us per step against the kernel's 27.6 -- is gone; its numbers are in profiles/r03*.)

        cbhg_kernel=True (HIP device; off by default): the encoder and the post-net run through `wrnn_taco_encode` / `wrnn_taco_postnet`
        (csrc/wrnn_cbhg.hip) instead of the torch ops; a state dict whose dims `wrnn_taco_front_create` refuses stays on the torch ops.
        `self.last_front_path` says which: 'hip' or 'torch'."""
        dev = self.device
        front = self._front_path(kernel, cbhg_kernel)
        seq, seq_proj = self.encode_kernel(ids)[:2] if front else self.encode(ids)
        if kernel:
            mel, attn = self._decode_kernel(seq, seq_proj, steps, kernel_variant)
            frames = [mel]
        else:
            n = seq.size(1)
            z = lambda *s: torch.zeros(*s, device=dev, dtype=seq.dtype)        # (a float64 state dict decodes in float64)
            st = dict(attn_h=z(1, self.decoder_dims), h1=z(1, self.lstm_dims), h2=z(1, self.lstm_dims), c1=z(1, self.lstm_dims),
                      c2=z(1, self.lstm_dims), context=z(1, self.decoder_dims), cumulative=z(1, n), attention=z(1, n))
            prenet_in = z(1, self.n_mels)                                          # the <GO> frame
            frames, scores_all = [], []
            for t in range(0, steps, self.r):
                m_, s_ = self._decoder_step(seq, seq_proj, prenet_in, st)
                frames.append(m_)
                scores_all.append(s_.clone())
                prenet_in = m_[:, :, -1]
                if (m_ < self.stop_threshold).all() and t > 10:
                    break
            attn = torch.cat([s.unsqueeze(-1).transpose(1, 2) for s in scores_all], 1)[0]
        mel = torch.cat(frames, dim=2)
        linear = self._postnet(mel, front)
        return mel[0].cpu().numpy(), linear.cpu().numpy(), attn.cpu().numpy()


def tacotron_to_wavernn_mel(mel):
    """gen_tacotron.py:143-145: rescale the Tacotron mel from [-4, 4] to [0, 1] and clip."""
    m = (np.asarray(mel) + 4) / 8
    return np.clip(m, 0, 1, out=m)
