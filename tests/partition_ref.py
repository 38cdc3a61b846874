"""An independent Python restatement of two rules of compute-engine_amd/csrc/tflite/lce_model.cc, written from the comments above
Partition(), FoldQuantize, ElementwiseChain and Bconv2d and sharing no code with them: (1) the epoch partition of a graph into
sections, and (2) which LceQuantize launches disappear into the launch in front of them, hence the counters the *_stats() entries
and run_stats()[1] report after a run.  It never calls the library.  No tests here.

A graph is described by plain lists: `ops[i] = (inputs, outputs)` (tensor indices; an absent optional input is -1), `kinds[i]` (one
of LCE_OPS, one of PASSES, or None for an operator no pass takes), the set `constants` of tensors with data in the file, and the
model's `outputs`."""

LCE_OPS = ("LceQuantize", "LceBconv2d", "LceBMaxPool2d", "LceDequantize")
HEADS = ("mean", "fully_connected", "softmax", "mean_i8", "fully_connected_i8", "softmax_i8")
# the seventeen fused passes, in the order of the library's table
PASSES = ("elementwise", "int8_add", "concat", "pool", "conv1x1", "depthwise", "conv2d", "conv_i8", "depthwise_i8") + HEADS + ("quantize", "dequantize")
# the passes whose launch can write the bits of an LceQuantize (a head and a float / int8 boundary never do)
FOLDING = PASSES[:9]
CHAIN_CAP = 8


def readers_of(ops):
    """tensor -> the operators that read it, once per input slot, in operator order."""
    readers = {}
    for i, (ins, _) in enumerate(ops):
        for t in ins:
            if t >= 0:
                readers.setdefault(t, []).append(i)
    return readers


def partition(ops, kinds, constants, outputs, stem):
    """The sections [(operators, inputs, outputs)] of the graph.  Epochs alternate between the LCE kind and the builtin kind,
    starting with the kind of the first ready operator in file order.  In an epoch every operator of its kind whose inputs are
    all made runs, until none is left.  An LCE operator and a head operator that a pass takes are of the LCE kind; an operator no
    pass takes is of the builtin kind; any other operator a pass takes has the kind of the epoch in which its last input is made
    -- ready from the start it is builtin, unless `stem` makes it LCE.  The LCE operators of one epoch, sorted, are a section."""
    n = len(ops)
    produced = {t for _, outs in ops for t in outs}
    made = set()
    kind = [1 if (kinds[i] in LCE_OPS or kinds[i] in HEADS) else (0 if kinds[i] is None else None) for i in range(n)]
    ready = lambda i: all(t < 0 or t not in produced or t in made for t in ops[i][0])
    start = [i for i in range(n) if ready(i)]
    for i in start:
        if kind[i] is None:
            kind[i] = 1 if stem else 0
    epoch = kind[start[0]] if start else 1
    left, idle, sections = set(range(n)), 0, []
    readers = readers_of(ops)
    while left and idle < 2:
        members, progress = [], True
        while progress:
            progress = False
            for i in sorted(left):
                if not ready(i):
                    continue
                if kind[i] is None:
                    kind[i] = epoch
                if kind[i] == epoch:
                    left.discard(i)
                    members.append(i)
                    made.update(ops[i][1])
                    progress = True
        if epoch == 1 and members:
            members.sort()
            inside = {t for i in members for t in ops[i][1]}
            ins = []
            for i in members:
                for t in ops[i][0]:
                    if t >= 0 and t not in constants and t not in inside and t not in ins:
                        ins.append(t)
            outs = [t for t in sorted(inside) if t in outputs or any(r not in members for r in readers.get(t, ()))]
            sections.append((members, ins, outs))
        idle = 0 if members else idle + 1
        epoch ^= 1
    return sections


def expected_counters(section, ops, kinds, constants, bit_tensors=()):
    """What one run of `section` = (operators, inputs, outputs) launches.  Returns {"passes": {pass: launches}, "folded": {pass:
    LceQuantize launches folded into it}, "ew_ops": ADD / MUL operators inside the elementwise launches, "conv_quantize": what
    run_stats()[1] reports, "chains": [(length, why it ended)]}.

    The walk is by file index and skips an operator a launch further up has covered.  THE fold rule: behind a pass whose last
    operator is `last` and whose result is `t`, the first LceQuantize of the section after `last` that reads `t` and has not run
    yet becomes the launch's bit output and does not launch (never behind a head, a boundary, or a join of bitpacked tensors:
    `bit_tensors`).  LceBconv2d has its own: of the LceQuantize operators of the section behind it that read its float / int8
    output, the first one does not launch.  An ADD / MUL chain starts at the first operator the walk meets and extends through
    the only reader of its result while that is an ADD / MUL of the section that has not run, the result is not delivered by the
    section, the step's tensor operand has been produced already, and the chain has fewer than CHAIN_CAP steps."""
    members, sec_in, sec_out = section
    inside = set(members)
    readers = readers_of(ops)
    done, have = set(), set(sec_in)
    launches, folded = {p: 0 for p in PASSES}, {p: 0 for p in PASSES}
    out = dict(passes=launches, folded=folded, ew_ops=0, conv_quantize=0, chains=[])

    def quantizes_behind(last, t):
        return [j for j in members if j > last and kinds[j] == "LceQuantize" and list(ops[j][0]) == [t]]

    def fold(name, last, t):
        launches[name] += 1
        if name in FOLDING and t not in bit_tensors:
            waiting = [j for j in quantizes_behind(last, t) if j not in done]
            if waiting:
                done.add(waiting[0])
                have.add(ops[waiting[0]][1][0])
                folded[name] += 1

    for i in members:
        if i in done:
            continue
        ins, outs = ops[i]
        name = kinds[i]
        if name == "elementwise":
            v = ins[1] if ins[0] in constants else ins[0]
            cur, length, why = i, 0, None
            while why is None:
                a, b = ops[cur][0]
                other = b if a == v else a
                if other not in constants and other not in have:
                    why = "operand"
                    break
                done.add(cur)
                length += 1
                last, v = cur, ops[cur][1][0]
                have.add(v)
                rd = readers.get(v, [])
                follows = len(rd) == 1 and v not in sec_out and kinds[rd[0]] == "elementwise" and rd[0] in inside and rd[0] not in done
                if not follows:
                    why = "end"
                elif length == CHAIN_CAP:
                    why = "cap"
                else:
                    cur = rd[0]
            assert length > 0
            out["ew_ops"] += length
            out["chains"].append((length, why))
            fold(name, last, v)
        elif name in PASSES:
            done.add(i)
            have.add(outs[0])
            fold(name, i, outs[0])
        else:
            have.add(outs[0])
            if name == "LceBconv2d" and outs[0] not in bit_tensors:
                behind = quantizes_behind(i, outs[0])
                for j in behind:
                    have.add(ops[j][1][0])
                if behind:
                    done.add(behind[0])
                    out["conv_quantize"] += 1
    return out
