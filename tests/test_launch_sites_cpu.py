"""One launch path: in segland_amd/csrc the runtime's kernel launch and its function-attribute call appear only inside the helpers that check them
(sl_launch in common.h, sl_lds_opt_in in api.cpp), and the last-error read only there and in sl_hip_clear_error.  A launch written by hand next to them would be a launch
nobody checks, or one checked under another kernel's name."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'segland_amd', 'csrc')
HOME = {'hipLaunchKernelGGL': {'sl_launch'}, 'hipFuncSetAttribute': {'sl_lds_opt_in'}, 'hipGetLastError': {'sl_launch', 'sl_hip_clear_error'}}


def sources():
    paths = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')) + [os.path.join(CSRC, 'api.cpp')])
    assert len(paths) >= 19, paths
    return paths


def code_of(path):
    """The file without // comments (a comment may name a call), offsets kept."""
    return re.sub(r'//[^\n]*', lambda m: ' ' * len(m.group(0)), open(path).read())


def definition_spans(text, name):
    """(start, end) of every definition `... name(...) {...}` in the text: from the name to the brace that closes its body."""
    spans = []
    for m in re.finditer(r'\b%s\s*\(' % name, text):
        i, depth = m.end(), 1
        while depth:                                   # the parameter list
            depth += {'(': 1, ')': -1}.get(text[i], 0)
            i += 1
        rest = re.match(r'\s*\{', text[i:])
        if not rest:
            continue                                   # a declaration or a call
        j, depth = i + rest.end(), 1
        while depth:
            depth += {'{': 1, '}': -1}.get(text[j], 0)
            j += 1
        spans.append((m.start(), j))
    return spans


def test_runtime_calls_only_inside_the_helpers():
    found = {call: 0 for call in HOME}
    stray = []
    for path in sources():
        text = code_of(path)
        for call, homes in HOME.items():
            spans = [s for h in homes for s in definition_spans(text, h)]
            for m in re.finditer(r'\b%s\b' % call, text):
                found[call] += 1
                if not any(a <= m.start() < b for a, b in spans):
                    stray.append('%s:%d %s' % (os.path.basename(path), text.count('\n', 0, m.start()) + 1, call))
        # nor the macro and the hand-kept opt-in flags that the helpers replaced
        assert 'SL_LAUNCH_CHECK' not in text, path
        assert not re.search(r'static\s+(bool|size_t)\s+(attr\w*|opted)\b', text), path
    assert not stray, 'launch / attribute / last-error calls outside sl_launch, sl_lds_opt_in and sl_hip_clear_error: %s' % stray
    assert found == {'hipLaunchKernelGGL': 1, 'hipFuncSetAttribute': 1, 'hipGetLastError': 2}, found
