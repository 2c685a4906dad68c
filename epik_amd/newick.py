"""A small Newick parser with the numbering of epik_amd/host/phylo_tree.hpp: post-order ids 0 .. N - 1 in the order of the
string, root = N - 1.  Reads what `SynthTree.newick()` and the usual tools write: labels (plain or 'quoted'), branch
lengths, [comments], jplace edge numbers `{id}`, any number of children a node."""
from __future__ import annotations

from dataclasses import dataclass, field


class NewickError(ValueError):
    pass


@dataclass
class Tree:
    parent: list = field(default_factory=list)      # -1 for the root
    children: list = field(default_factory=list)    # ids, in the order of the string
    length: list = field(default_factory=list)      # float, None where the string gives none
    label: list = field(default_factory=list)       # "" where the string gives none
    edge: list = field(default_factory=list)        # the jplace number `{id}` of the edge above, None without

    @property
    def num_nodes(self) -> int:
        return len(self.parent)

    @property
    def root(self) -> int:
        return len(self.parent) - 1

    def is_leaf(self, i: int) -> bool:
        return not self.children[i]

    def leaves(self) -> list:
        return [i for i in range(self.num_nodes) if not self.children[i]]

    def neighbours(self) -> list:
        """The tree without its rooting: per node the nodes one edge away."""
        out = [list(c) for c in self.children]
        for i, p in enumerate(self.parent):
            if p >= 0:
                out[i].append(p)
        return out


def _fail(text: str, at: int, what: str):
    line = text.count("\n", 0, at) + 1
    raise NewickError(f"Newick, line {line}, character {at - (text.rfind(chr(10), 0, at) + 1) + 1}: {what}")


def parse(text: str) -> Tree:
    tree = Tree()
    open_nodes = []     # per open bracket the ids of the children read so far
    pending = []        # the children of the node whose label comes next (after a closing bracket)
    i, n = 0, len(text)
    done = False

    def add(children, label, length, edge):
        node = tree.num_nodes
        tree.parent.append(-1)
        tree.children.append(list(children))
        tree.length.append(length)
        tree.label.append(label)
        tree.edge.append(edge)
        for c in children:
            tree.parent[c] = node
        return node

    expect_node = True  # a node (leaf label or bracket) may start here
    while i < n:
        ch = text[i]
        if ch.isspace():
            i += 1
        elif ch == "[":
            end = text.find("]", i)
            if end < 0:
                _fail(text, i, "a comment that does not end")
            i = end + 1
        elif done:
            _fail(text, i, "text after the final ';'")
        elif ch == "(":
            if not expect_node:
                _fail(text, i, "'(' where ',' or ')' should be")
            open_nodes.append([])
            i += 1
        elif ch == ";":
            if open_nodes or tree.num_nodes == 0 or expect_node:
                _fail(text, i, "';' before the tree is closed")
            done = True
            i += 1
        elif ch == "," and not expect_node:
            if not open_nodes:
                _fail(text, i, "',' outside every bracket")
            expect_node = True
            i += 1
        elif ch == ")" and not expect_node:
            if not open_nodes:
                _fail(text, i, "')' without '('")
            pending = open_nodes.pop()
            i += 1
            i = _node_tail(text, i, tree, add, pending, open_nodes)
        elif expect_node and ch not in ",)":
            i = _node_tail(text, i, tree, add, [], open_nodes)
            expect_node = False
        else:
            _fail(text, i, f"'{ch}' where a node should be")
    if not done:
        _fail(text, max(n - 1, 0), "no final ';'")
    return tree


def _node_tail(text, i, tree, add, children, open_nodes) -> int:
    """label[:length][{edge}] of a node whose children are read; the node is added, the position after it returned."""
    n = len(text)
    label = ""
    if i < n and text[i] == "'":
        end = i + 1
        parts = []
        while True:
            nxt = text.find("'", end)
            if nxt < 0:
                _fail(text, i, "a quoted label that does not end")
            parts.append(text[end:nxt])
            if nxt + 1 < n and text[nxt + 1] == "'":  # '' inside quotes is one quote
                parts.append("'")
                end = nxt + 2
                continue
            i = nxt + 1
            break
        label = "".join(parts)
    else:
        start = i
        while i < n and text[i] not in "(),:;[]{}'" and not text[i].isspace():
            i += 1
        label = text[start:i]
    length, edge = None, None
    while i < n and text[i].isspace():
        i += 1
    if i < n and text[i] == ":":
        start = i + 1
        i = start
        while i < n and text[i] not in "(),:;[]{}" and not text[i].isspace():
            i += 1
        try:
            length = float(text[start:i])
        except ValueError:
            _fail(text, start, f"'{text[start:i]}' is no branch length")
    if i < n and text[i] == "{":
        end = text.find("}", i)
        if end < 0 or not text[i + 1:end].strip().isdigit():
            _fail(text, i, "'{' that is no jplace edge number")
        edge = int(text[i + 1:end])
        i = end + 1
    node = add(children, label, length, edge)
    if open_nodes:
        open_nodes[-1].append(node)
    return i


def _quoted(label: str) -> str:
    if label and any(c in label for c in "(),:;[]{}' \t\n"):
        return "'" + label.replace("'", "''") + "'"
    return label


def write(tree: Tree, lengths: bool = True, edges: bool = False, root: int | None = None) -> str:
    """The tree as one line of Newick, children in their order."""
    root = tree.root if root is None else root
    out = []
    stack = [(root, 0)]
    while stack:
        node, at = stack.pop()
        kids = tree.children[node]
        if at == 0 and kids:
            out.append("(")
        if at < len(kids):
            if at:
                out.append(",")
            stack.append((node, at + 1))
            stack.append((kids[at], 0))
            continue
        if kids:
            out.append(")")
        out.append(_quoted(tree.label[node]))
        if lengths and tree.length[node] is not None and node != root:
            out.append(f":{tree.length[node]:.17g}")
        if edges and node != root:
            out.append("{%d}" % node)
    return "".join(out) + ";"
