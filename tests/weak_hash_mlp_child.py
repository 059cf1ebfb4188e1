"""The process that runs the fused value-guided greedy search of tests/test_gpu_fused_vgreedy.py
through libacx_weakhash.so: tests/weak_hash_child.py with one more `op`.

    ACX_LIB=<variant> python tests/weak_hash_mlp_child.py <dir>

vgreedy_mlp_many: acx.value_guided_greedy_search_many scored by the acx.DeviceMLP mlp_common.net(kind,
hidden) with its normalisation, fused or stepped; the nodes whose key hashes are counted are the
yardstick's, scored by mlp.host."""
import weak_hash_child as C


class Ops(C.Ops):
    def vgreedy_mlp_many(self, i, c):
        import acx
        import mlp_common as MC
        import vgreedy_yardstick as Y
        mlp, mean, std = MC.net(c["kind"], tuple(c["hidden"]))
        return self._scored_many(acx.value_guided_greedy_search_many, c,
                                 lambda p, j: Y.vgreedy(p, mlp.host, c["budgets"][j], c["cyc"], mean=mean, std=std,
                                                        drop_twins=True),
                                 scorer=mlp, max_nodes_to_explore=c["budgets"], feat_mean=mean, feat_std=std,
                                 fused=c["fused"])


if __name__ == "__main__":
    C.Ops = Ops
    C.main()
