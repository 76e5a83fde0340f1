"""The refusals of the Tacotron decoder's entry points, word for word, without a GPU: `wrnn_taco_decode_batch`, `wrnn_taco_decode_forced`, their
`_groups` forms (csrc/wrnn_taco_batch.hip) and the geometry check they share with `wrnn_taco_decode` (csrc/wrnn_taco.hip).  Every row pins the
return code and the FULL text of `wrnn_taco_last_error()` -- through the plain entry, through the groups entry with one group (the plain call's
text) and with two (the same text behind "group g: ") -- and the order in which the checks are made.  The strings are what the library answered
before the four entry points shared their checks; a change of the host code must leave every one of them as it is.  All pointers are fakes the
checks never follow; device 10000 does not exist, so a call that got past its checks would come back with another code than WRNN_ERR_ARG."""
import ctypes
import os

import pytest

FAKE = 0x10000                                                           # a non-null "device pointer"
WS0, WS1 = 0x10000000, 0x20000000                                        # two "workspaces" far apart
NO_DEVICE = 10_000
FREE_BYTES, FORCED_BYTES = 185376, 217632                                # the workspaces of the two-sentence calls below


def _lib_or_build():
    from wavernn_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib, _lib.lib()


def _weights(_lib):
    w = _lib.TacoWeights()
    w.struct_bytes = ctypes.sizeof(_lib.TacoWeights)
    w.n_mels, w.prenet1, w.prenet2, w.decoder_dims, w.encoder_width, w.lstm_dims, w.attn_filters, w.attn_kernel = 80, 256, 128, 256, 256, 512, 32, 31
    for name in _lib.TACO_WEIGHT_FIELDS:
        setattr(w, name, FAKE)
    return w


def _free(_lib, L, workspace=WS0, r=1, max_r=2):
    c = _lib.TacoBatchCall()
    c.struct_bytes = ctypes.sizeof(_lib.TacoBatchCall)
    c.n_sent, c.r, c.max_r, c.stop_threshold = 2, r, max_r, -3.4
    c.n, c.max_steps = (ctypes.c_int32 * 2)(74, 12), (ctypes.c_int32 * 2)(40, 40)
    for name in ('seq', 'seq_proj', 'mel_out', 'scores_out'):
        setattr(c, name, (ctypes.c_void_p * 2)(FAKE, FAKE))
    c.steps_done, c.workspace = FAKE, workspace
    c.workspace_bytes = L.wrnn_taco_batch_workspace_bytes(2)
    return c


def _forced(_lib, L, workspace=WS0, r=1, max_r=2):
    c = _lib.TacoForcedCall()
    c.struct_bytes = ctypes.sizeof(_lib.TacoForcedCall)
    c.n_sent, c.r, c.max_r = 2, r, max_r
    c.n, c.frames = (ctypes.c_int32 * 2)(74, 12), (ctypes.c_int32 * 2)(40, 23)
    for name in ('seq', 'seq_proj', 'force_mel', 'mel_out', 'scores_out'):
        setattr(c, name, (ctypes.c_void_p * 2)(FAKE, FAKE))
    c.workspace = workspace
    c.workspace_bytes = L.wrnn_taco_forced_workspace_bytes(2, c.frames, r)
    return c


FORMS = {'free': ('wrnn_taco_decode_batch', 'wrnn_taco_decode_batch_groups', 'TacoBatchCall', _free),
         'forced': ('wrnn_taco_decode_forced', 'wrnn_taco_decode_forced_groups', 'TacoForcedCall', _forced)}


def _plain(_lib, L, form, w, c):
    rc = getattr(L, FORMS[form][0])(NO_DEVICE, ctypes.byref(w) if w is not None else None, ctypes.byref(c) if c is not None else None)
    return rc, L.wrnn_taco_last_error().decode()


def _groups(_lib, L, form, w, calls, n_groups=None):
    struct = getattr(_lib, FORMS[form][2])
    table = (ctypes.POINTER(struct) * len(calls))(*[ctypes.pointer(c) if c is not None else None for c in calls]) if calls is not None else None
    rc = getattr(L, FORMS[form][1])(NO_DEVICE, ctypes.byref(w) if w is not None else None, table, len(calls) if n_groups is None else n_groups)
    return rc, L.wrnn_taco_last_error().decode()


# ---- the edits that make a valid call a refused one ----
def _set(**fields):
    def edit(c, w):
        for k, v in fields.items():
            setattr(c, k, v)
    return edit


def _set_w(**fields):
    def edit(c, w):
        for k, v in fields.items():
            setattr(w, k, v)
    edit.on_weights = True                                               # (the weights are every group's: group 0 reports the fault)
    return edit


def _shrink(which):
    def edit(c, w):
        (c if which == 'call' else w).struct_bytes -= 4
    edit.on_weights = which != 'call'
    return edit


def _entry(table, s, v):
    def edit(c, w):
        getattr(c, table)[s] = v
    return edit


def _null_table(table):
    def edit(c, w):
        setattr(c, table, ctypes.cast(None, type(getattr(c, table))))
    return edit


def _short(c, w):
    c.workspace_bytes -= 1


SIZE = 'struct size mismatch (header / library versions differ)'
R = 'r=%d max_r=%d: frames per step must be 1..min(max_r, 8)'
N_SENT = 'n_sent=%d: a call decodes 1..8 sentences (WRNN_TACO_BATCH_MAX)'
GEOMETRY = "unsupported decoder geometry (the kernel is built for the reference's hparams: 80 / 256 / 128 / 256 / 512 / 32 x 31)"
FREE_NULL = 'null buffer: n, max_steps, seq, seq_proj, mel_out, scores_out, steps_done and workspace are all required'
FREE_N = 'sentence 1: n=%d encoder positions, the batched kernel takes 1..256 (WRNN_TACO_BATCH_NMAX; longer: wrnn_taco_decode)'
FREE_ENTRY = 'sentence %d: null buffer (seq, seq_proj, mel_out and scores_out are required)'
FORCED_NULL = 'null buffer: n, frames, seq, seq_proj, force_mel, mel_out, scores_out and workspace are all required'
FORCED_N = 'sentence 1: n=%d encoder positions, the forced kernel takes 1..256 (WRNN_TACO_BATCH_NMAX)'
FORCED_ENTRY = 'sentence %d: null buffer (seq, seq_proj, force_mel, mel_out and scores_out are required)'

# (edit, the message behind the prefix), in the order of the checks; an edit of the weights is every group's, so group 0 reports it
COMMON = [(_shrink('call'), SIZE), (_shrink('weights'), SIZE),
          (_set(n_sent=0), N_SENT % 0), (_set(n_sent=9), N_SENT % 9), (_set(n_sent=-3), N_SENT % -3),
          (_set(r=0), R % (0, 2)), (_set(r=3), R % (3, 2)), (_set(r=9, max_r=20), R % (9, 20)), (_set(r=-1, max_r=-1), R % (-1, -1))]
GEOM = [(_set_w(**{k: v}), GEOMETRY) for k, v in (('n_mels', 40), ('prenet1', 128), ('prenet2', 256), ('decoder_dims', 128), ('encoder_width', 512),
                                                    ('lstm_dims', 256), ('attn_filters', 16), ('attn_kernel', 15))]
ROWS = {
    'free': COMMON +
    [(_null_table(t), FREE_NULL) for t in ('n', 'max_steps', 'seq', 'seq_proj', 'mel_out', 'scores_out')] +
    [(_set(steps_done=None), FREE_NULL), (_set(workspace=None), FREE_NULL),
     (_entry('n', 1, 0), FREE_N % 0), (_entry('n', 1, 257), FREE_N % 257), (_entry('n', 1, -7), FREE_N % -7),
     (_entry('max_steps', 0, 0), 'sentence 0: max_steps=0, at least 1'), (_entry('max_steps', 1, -5), 'sentence 1: max_steps=-5, at least 1')] +
    [(_entry(t, s, None), FREE_ENTRY % s) for s, t in enumerate(('seq', 'seq_proj'))] +
    [(_entry(t, 1 - s, None), FREE_ENTRY % (1 - s)) for s, t in enumerate(('mel_out', 'scores_out'))] +
    [(_short, f'workspace of {FREE_BYTES - 1} bytes, 2 sentences need {FREE_BYTES} (wrnn_taco_batch_workspace_bytes)'),
     (_set(workspace_bytes=0), f'workspace of 0 bytes, 2 sentences need {FREE_BYTES} (wrnn_taco_batch_workspace_bytes)')] + GEOM,
    'forced': COMMON +
    [(_null_table(t), FORCED_NULL) for t in ('n', 'frames', 'seq', 'seq_proj', 'force_mel', 'mel_out', 'scores_out')] +
    [(_set(workspace=None), FORCED_NULL),
     (_entry('n', 1, 0), FORCED_N % 0), (_entry('n', 1, 257), FORCED_N % 257), (_entry('n', 1, -7), FORCED_N % -7),
     (_entry('frames', 0, 0), 'sentence 0: frames=0 ground-truth frames, 1..1048576'),
     (_entry('frames', 1, (1 << 20) + 1), 'sentence 1: frames=1048577 ground-truth frames, 1..1048576')] +
    [(_entry(t, s % 2, None), FORCED_ENTRY % (s % 2)) for s, t in enumerate(('seq', 'seq_proj', 'force_mel', 'mel_out', 'scores_out'))] +
    [(_short, f'workspace of {FORCED_BYTES - 1} bytes, these 2 sentences need {FORCED_BYTES} (wrnn_taco_forced_workspace_bytes)'),
     (_set(workspace_bytes=0), f'workspace of 0 bytes, these 2 sentences need {FORCED_BYTES} (wrnn_taco_forced_workspace_bytes)')] + GEOM,
}
CASES = [(form, i) for form in ROWS for i in range(len(ROWS[form]))]


@pytest.mark.parametrize('form,row', CASES, ids=[f'{form}-{i}' for form, i in CASES])
def test_a_refusal_has_the_same_words_through_every_entry(form, row):
    _lib, L = _lib_or_build()
    make = FORMS[form][3]
    edit, text = ROWS[form][row]
    on_weights = getattr(edit, 'on_weights', False)
    # the plain entry, and the groups entry with one group: the plain call's message, without a group in front
    w, c = _weights(_lib), make(_lib, L)
    edit(c, w)
    assert _plain(_lib, L, form, w, c) == (_lib.ERR_ARG, text)
    assert _groups(_lib, L, form, w, [c]) == (_lib.ERR_ARG, text)
    # two groups: the group that has the fault in front
    for g in (0, 1):
        w, calls = _weights(_lib), [make(_lib, L, workspace=WS0), make(_lib, L, workspace=WS1)]
        edit(calls[g], w)
        assert _groups(_lib, L, form, w, calls) == (_lib.ERR_ARG, f'group {0 if on_weights else g}: {text}')


@pytest.mark.parametrize('form', list(FORMS))
def test_the_workspace_sizes_the_messages_quote(form):
    _lib, L = _lib_or_build()
    assert FORMS[form][3](_lib, L).workspace_bytes == (FREE_BYTES if form == 'free' else FORCED_BYTES)


@pytest.mark.parametrize('form', list(FORMS))
def test_null_arguments(form):
    _lib, L = _lib_or_build()
    make = FORMS[form][3]
    w, c = _weights(_lib), make(_lib, L)
    assert _plain(_lib, L, form, None, c) == (_lib.ERR_ARG, 'null argument')
    assert _plain(_lib, L, form, w, None) == (_lib.ERR_ARG, 'null argument')
    assert _plain(_lib, L, form, None, None) == (_lib.ERR_ARG, 'null argument')
    assert _groups(_lib, L, form, None, [c]) == (_lib.ERR_ARG, 'null argument')
    assert _groups(_lib, L, form, None, [make(_lib, L, workspace=WS0), make(_lib, L, workspace=WS1)]) == (_lib.ERR_ARG, 'group 0: null argument')


@pytest.mark.parametrize('form', list(FORMS))
def test_the_groups_table_refusals(form):
    _lib, L = _lib_or_build()
    make = FORMS[form][3]
    w = _weights(_lib)
    pair = lambda: [make(_lib, L, workspace=WS0), make(_lib, L, workspace=WS1)]
    for n_groups in (0, -1, 3):
        assert _groups(_lib, L, form, w, pair(), n_groups=n_groups) == (_lib.ERR_ARG, f'n_groups={n_groups}: a call decodes 1..2 groups (WRNN_TACO_GROUPS_MAX)')
    assert _groups(_lib, L, form, None, None, n_groups=5) == (_lib.ERR_ARG, 'n_groups=5: a call decodes 1..2 groups (WRNN_TACO_GROUPS_MAX)')
    for n_groups in (1, 2):
        assert _groups(_lib, L, form, w, None, n_groups=n_groups) == (_lib.ERR_ARG, f'null argument: calls is a table of n_groups={n_groups} call structs')
    null = 'group %d: null call (calls[0 .. n_groups) are all required)'
    assert _groups(_lib, L, form, w, [None]) == (_lib.ERR_ARG, null % 0)
    assert _groups(_lib, L, form, w, [None, make(_lib, L)]) == (_lib.ERR_ARG, null % 0)
    assert _groups(_lib, L, form, w, [make(_lib, L), None]) == (_lib.ERR_ARG, null % 1)
    assert _groups(_lib, L, form, w, [None, None]) == (_lib.ERR_ARG, null % 0)
    # the table comes before the calls: a null entry is reported though the other call is a bad one, and though the weights are null
    bad = make(_lib, L)
    bad.n_sent = 9
    assert _groups(_lib, L, form, w, [bad, None]) == (_lib.ERR_ARG, null % 1)
    assert _groups(_lib, L, form, None, [bad, None]) == (_lib.ERR_ARG, null % 1)


@pytest.mark.parametrize('form', list(FORMS))
def test_the_groups_pair_refusals(form):
    _lib, L = _lib_or_build()
    make = FORMS[form][3]
    w = _weights(_lib)
    size = FREE_BYTES if form == 'free' else FORCED_BYTES
    # one stream
    calls = [make(_lib, L, workspace=WS0), make(_lib, L, workspace=WS1)]
    calls[0].stream, calls[1].stream = 0x80, 0x40
    assert _groups(_lib, L, form, w, calls) == (_lib.ERR_ARG, 'group 1: stream 0x40, group 0 has 0x80: the groups of a call ride ONE launch on one stream')
    # one r, one max_r
    share = 'group 1: r=%d max_r=%d, group 0 has r=%d max_r=%d: the groups of a call share the weights, so r and max_r are equal'
    calls = [make(_lib, L, workspace=WS0, r=1, max_r=2), make(_lib, L, workspace=WS1, r=2, max_r=2)]
    assert _groups(_lib, L, form, w, calls) == (_lib.ERR_ARG, share % (2, 2, 1, 2))
    calls = [make(_lib, L, workspace=WS0, r=1, max_r=2), make(_lib, L, workspace=WS1, r=1, max_r=3)]
    assert _groups(_lib, L, form, w, calls) == (_lib.ERR_ARG, share % (1, 3, 1, 2))
    # the stream comes before r
    calls = [make(_lib, L, workspace=WS0, r=1, max_r=2), make(_lib, L, workspace=WS1, r=2, max_r=2)]
    calls[1].stream = 0x40
    calls[0].stream = 0x80
    assert _groups(_lib, L, form, w, calls)[1].startswith('group 1: stream 0x40, group 0 has 0x80')
    # workspaces of their own: the same one, one byte of overlap at either end
    overlap = 'the workspaces of group 0 (%d bytes at 0x%x) and group 1 (%d bytes at 0x%x) overlap: every group needs a workspace of its own'
    for ws1 in (WS0, WS0 + size - 1, WS0 - size + 1):
        calls = [make(_lib, L, workspace=WS0), make(_lib, L, workspace=ws1)]
        assert _groups(_lib, L, form, w, calls) == (_lib.ERR_ARG, overlap % (size, WS0, size, ws1))
    calls = [make(_lib, L, workspace=WS0), make(_lib, L, workspace=WS0 + 8)]
    calls[1].workspace_bytes += 24                                       # (a larger workspace than needed is a valid one)
    assert _groups(_lib, L, form, w, calls) == (_lib.ERR_ARG, overlap % (size, WS0, size + 24, WS0 + 8))
    # r before the workspaces; every call's own checks before the pair's
    calls = [make(_lib, L, workspace=WS0, r=1, max_r=2), make(_lib, L, workspace=WS0, r=2, max_r=2)]
    assert _groups(_lib, L, form, w, calls) == (_lib.ERR_ARG, share % (2, 2, 1, 2))
    calls = [make(_lib, L, workspace=WS0), make(_lib, L, workspace=WS0)]
    calls[1].stream = 0x40
    calls[1].n[0] = 300
    assert _groups(_lib, L, form, w, calls)[1].startswith('group 1: sentence 0: n=300 encoder positions')
    # adjacent workspaces are fine: the call gets past its checks and it is the DEVICE that refuses
    calls = [make(_lib, L, workspace=WS0), make(_lib, L, workspace=WS0 + size)]
    assert _groups(_lib, L, form, w, calls)[0] not in (_lib.WRNN_OK, _lib.ERR_ARG)


@pytest.mark.parametrize('form', list(FORMS))
def test_the_checks_of_a_call_keep_their_order(form):
    """Rows i < j of ROWS together: row i's message (the rows are in the order of the checks).  Per sentence the order is n, steps, buffers, so an
    earlier sentence's later check comes before a later sentence's earlier one."""
    _lib, L = _lib_or_build()
    make = FORMS[form][3]
    steps, entry = ('max_steps', FREE_ENTRY) if form == 'free' else ('frames', FORCED_ENTRY)
    firsts = [(_shrink('call'), SIZE), (_set(n_sent=0), N_SENT % 0), (_set(r=0), R % (0, 2))]
    null_table = (_null_table('seq_proj'), FREE_NULL if form == 'free' else FORCED_NULL)
    n1 = (_entry('n', 1, 257), (FREE_N if form == 'free' else FORCED_N) % 257)
    steps0 = (_entry(steps, 0, 0), 'sentence 0: max_steps=0, at least 1' if form == 'free' else 'sentence 0: frames=0 ground-truth frames, 1..1048576')
    steps1 = (_entry(steps, 1, 0), steps0[1].replace('sentence 0', 'sentence 1'))
    entry0, entry1 = (_entry('mel_out', 0, None), entry % 0), (_entry('mel_out', 1, None), entry % 1)
    short = [row for row in ROWS[form] if row[0] is _short][0]
    geometry = (_set_w(attn_kernel=15), GEOMETRY)
    chain = firsts + [null_table, steps0, entry0, n1, steps1, entry1, short, geometry]
    for i in range(len(chain)):
        for g in (None, 0, 1):
            if g == 1 and chain[i] is geometry:                          # (the weights are group 0's too: below)
                continue
            w, calls = _weights(_lib), [make(_lib, L, workspace=WS0), make(_lib, L, workspace=WS1)]
            c = calls[g or 0]
            for edit, _ in reversed(chain[i:] if g != 1 else chain[i:-1]):   # (the later faults first: the edit of n_sent comes last)
                edit(c, w)
            if g is None:
                assert _plain(_lib, L, form, w, c) == (_lib.ERR_ARG, chain[i][1]), i
            else:
                assert _groups(_lib, L, form, w, calls) == (_lib.ERR_ARG, f'group {g}: {chain[i][1]}'), (i, g)
    # two groups: group 0's last check (the geometry) comes before group 1's first
    w, calls = _weights(_lib), [make(_lib, L, workspace=WS0), make(_lib, L, workspace=WS1)]
    w.lstm_dims = 256
    calls[1].n_sent = 0
    assert _groups(_lib, L, form, w, calls) == (_lib.ERR_ARG, 'group 0: ' + GEOMETRY)


def test_the_single_sentence_decoder_refuses_the_same_geometry_in_the_same_words():
    _lib, L = _lib_or_build()

    def call():
        c = _lib.TacoCall()
        c.struct_bytes = ctypes.sizeof(_lib.TacoCall)
        c.n, c.r, c.max_r, c.max_steps, c.stop_threshold = 12, 1, 2, 5, -3.4
        c.seq = c.seq_proj = c.mel_out = c.scores_out = c.steps_done = c.workspace = FAKE
        c.workspace_bytes = L.wrnn_taco_workspace_bytes()
        return c

    def run(w, c):
        rc = L.wrnn_taco_decode(NO_DEVICE, ctypes.byref(w) if w is not None else None, ctypes.byref(c) if c is not None else None)
        return rc, L.wrnn_taco_last_error().decode()
    for k, v in (('n_mels', 40), ('prenet1', 128), ('prenet2', 256), ('decoder_dims', 128), ('encoder_width', 512), ('lstm_dims', 256),
                 ('attn_filters', 16), ('attn_kernel', 15)):
        w = _weights(_lib)
        setattr(w, k, v)
        assert run(w, call()) == (_lib.ERR_ARG, GEOMETRY), k
    # ... after its own checks of the call
    w = _weights(_lib)
    w.lstm_dims = 256
    assert run(None, call()) == (_lib.ERR_ARG, 'null argument') and run(w, None) == (_lib.ERR_ARG, 'null argument')
    c = call()
    c.struct_bytes -= 4
    assert run(w, c) == (_lib.ERR_ARG, SIZE)
    c = call()
    c.n = 1025
    assert run(w, c) == (_lib.ERR_ARG, 'bad call: n=1025 (1..1024) r=1 max_r=2 max_steps=5 or a null / short buffer')
    c = call()
    c.workspace_bytes -= 1
    assert run(w, c) == (_lib.ERR_ARG, 'bad call: n=12 (1..1024) r=1 max_r=2 max_steps=5 or a null / short buffer')
    # valid arguments: past the checks, and the DEVICE refuses
    assert run(_weights(_lib), call())[0] not in (_lib.WRNN_OK, _lib.ERR_ARG)
