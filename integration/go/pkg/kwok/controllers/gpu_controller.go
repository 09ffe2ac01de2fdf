//go:build kwok_mi355x

// gpu_controller.go - the client-go side of the drop-in: watch events are
// batched, encoded as object JSON, decoded by the engine's host codec and
// ingested before each tick; every body the tick returns is applied through the
// clientset with the reference's 16-wide task pools (utils.go:119-161).  The
// watch echoes of the engine's own patches are dropped by resourceVersion
// (echoes).  kwok_amd/controller.py is the same controller in Python, which
// the tests run against a fake clientset (tests/test_controller*.py).
// NewController builds this in place of NodeController + PodController when
// the package is built with -tags kwok_mi355x (controller_mi355x.go).
//
// Not compiled in this repository (no Go toolchain in the image).

package controllers

/*
#include "kwok_engine.h"
#include "kwok_watch.h"
*/
import "C"

import (
	"bytes"
	"context"
	"encoding/binary"
	"encoding/json"
	"fmt"
	"net"
	"os"
	"runtime"
	"sync"
	"time"

	corev1 "k8s.io/api/core/v1"
	apierrors "k8s.io/apimachinery/pkg/api/errors"
	metav1 "k8s.io/apimachinery/pkg/apis/meta/v1"
	"k8s.io/apimachinery/pkg/types"
	"k8s.io/apimachinery/pkg/watch"
	"k8s.io/client-go/kubernetes/scheme"

	"sigs.k8s.io/kwok/pkg/cni"
	"sigs.k8s.io/kwok/pkg/log"
)

// watchObj: one watch event since the last tick.  The object is encoded to
// JSON only at the next tick, after the echoes of the engine's own patches are
// dropped (echoes).
type watchObj struct {
	obj     interface{}
	uid     types.UID
	rv      string // metadata.resourceVersion
	deleted bool
}

// objBatch: the watch objects of one tick as concatenated JSON (the codec's input)
type objBatch struct {
	arena []byte
	offs  []uint64
	lens  []uint32
	del   []bool
	uids  []types.UID
	refs  []types.NamespacedName // namespace / name (a pod's: the apply's target; a node's name)
	nodes []string               // pods: spec.nodeName (EnableCNI's cni.Remove check)
}

func (b *objBatch) add(w watchObj) error {
	raw, err := json.Marshal(w.obj)
	if err != nil {
		return err
	}
	b.offs = append(b.offs, uint64(len(b.arena)))
	b.lens = append(b.lens, uint32(len(raw)))
	b.arena = append(b.arena, raw...)
	b.del = append(b.del, w.deleted)
	b.uids = append(b.uids, w.uid)
	var ref types.NamespacedName // (one entry per object, so the indices stay aligned)
	var node string
	switch o := w.obj.(type) {
	case *corev1.Pod:
		ref, node = types.NamespacedName{Namespace: o.Namespace, Name: o.Name}, o.Spec.NodeName
	case *corev1.Node:
		ref = types.NamespacedName{Name: o.Name}
	}
	b.refs = append(b.refs, ref)
	b.nodes = append(b.nodes, node)
	return nil
}

// echoes: the resourceVersions the engine's own patches returned, per object.
// Their Modified watch events (the echoes) are states the engine already
// assumed when it emitted the patches (DESIGN.md §1: patches are assumed
// applied; a heartbeat's echo re-lock, node_controller.go:152 -> :256-263, is
// part of every tick), so echoes are dropped instead of re-ingested.  An object
// can take several patches in one tick (a node's heartbeat and its init patch,
// a pod's finalizer patch), each with its own echo: every returned version is
// kept until its echo is seen (the last echoKeep per object, so echoes lost to a
// watch restart do not pile up).  Any other event of the object is ingested.
//
// ledger (KWOK_ECHO_LEDGER=1, with KWOK_UID_DIR=1): the engine's echo ledger (kwok_watch.h, DESIGN.md §24)
// holds the notes in HBM.  note / forget then only queue their op, in call order; flush sends the queue
// with one kwok_echo_update; every decision is taken at flush by kwok_echo_match under the same rule
// (is answers false: nothing is dropped on arrival) and rv stays empty.
type echoes struct {
	mu sync.Mutex
	rv map[types.UID][]string

	ledger *gpuEngine
	ops    []uint8
	uids   []string
	rvs    []string
}

const echoKeep = 8

func (x *echoes) note(uid types.UID, rv string) {
	if uid == "" || rv == "" {
		return
	}
	x.mu.Lock()
	if x.ledger != nil {
		x.ops, x.uids, x.rvs = append(x.ops, echoNote), append(x.uids, string(uid)), append(x.rvs, rv)
		x.mu.Unlock()
		return
	}
	v := append(x.rv[uid], rv)
	if len(v) > echoKeep {
		v = v[1:]
	}
	x.rv[uid] = v
	x.mu.Unlock()
}

// is: the event is the echo of one of the engine's patches of the object (each
// echo is consumed: a second event with that resourceVersion is not expected)
func (x *echoes) is(uid types.UID, rv string) bool {
	x.mu.Lock()
	defer x.mu.Unlock()
	if x.ledger != nil { // decided at flush, on the device
		return false
	}
	v := x.rv[uid]
	for i, r := range v {
		if r == rv {
			v = append(v[:i], v[i+1:]...)
			if len(v) == 0 {
				delete(x.rv, uid)
			} else {
				x.rv[uid] = v
			}
			return true
		}
	}
	return false
}

func (x *echoes) forget(uid types.UID) {
	x.mu.Lock()
	if x.ledger != nil {
		if uid != "" {
			x.ops, x.uids, x.rvs = append(x.ops, echoForget), append(x.uids, string(uid)), append(x.rvs, "")
		}
	} else {
		delete(x.rv, uid)
	}
	x.mu.Unlock()
}

// flush (ledger): the queued notes and forgets in one kwok_echo_update, applied in queue order per uid.
// Called when every apply of the previous tick has returned, before the batches are filtered
func (x *echoes) flush() error {
	x.mu.Lock()
	ops, uids, rvs := x.ops, x.uids, x.rvs
	x.ops, x.uids, x.rvs = nil, nil, nil
	x.mu.Unlock()
	if x.ledger == nil || len(ops) == 0 {
		return nil
	}
	return x.ledger.echoUpdate(ops, uids, rvs)
}

// encode drops the echoes among ws (those whose patch returned after the watch
// event arrived: onEvent could not match them yet) and encodes the rest
func (x *echoes) encode(ws []watchObj) (objBatch, int, error) {
	var b objBatch
	dropped := 0
	if x.ledger != nil && len(ws) > 0 { // the same rule, decided by the device ledger (kwok_echo_match)
		uids, rvs, del := make([]string, len(ws)), make([]string, len(ws)), make([]bool, len(ws))
		for i, w := range ws {
			uids[i], rvs[i], del[i] = string(w.uid), w.rv, w.deleted
		}
		drop, err := x.ledger.echoMatch(uids, rvs, del)
		if err != nil {
			return b, 0, err
		}
		for i, w := range ws {
			if drop[i] != 0 {
				dropped++
				continue
			}
			if err := b.add(w); err != nil {
				return b, dropped, err
			}
		}
		return b, dropped, nil
	}
	seen := map[types.UID]struct{}{} // (the rule of onEvent: only before any kept event of the object)
	for _, w := range ws {
		_, after := seen[w.uid]
		if !w.deleted && x.is(w.uid, w.rv) && !after {
			dropped++
			continue
		}
		seen[w.uid] = struct{}{}
		if err := b.add(w); err != nil {
			return b, dropped, err
		}
		if w.deleted { // the object's last event: echoes still noted for it will not come
			x.forget(w.uid)
		}
	}
	return b, dropped, nil
}

// GPUController: one engine (one GPU) behind the reference's Controller API.
type GPUController struct {
	conf      Config
	eng       *gpuEngine
	codec     *gpuCodec
	interval  time.Duration
	finalizer []byte

	mu    sync.Mutex // guards the batches (watch goroutines append, the tick loop swaps)
	nodes  []watchObj
	pods   []watchObj
	queued map[types.UID]struct{} // objects with an event in the batches
	echo   echoes

	// tick loop only
	nodeName   map[int32]string // node handle -> name
	nodeHandle map[string]int32 // name -> node handle (nodes the engine holds; pods name them by handle)
	podByUID   map[types.UID]int32
	podUID   map[int32]types.UID // pod handle -> UID (the reverse of podByUID)
	podRef   map[int32]types.NamespacedName

	// byUID (KWOK_UID_DIR=1): the engine's pod uid directory (kwok_watch.h, DESIGN.md §23) holds uid -> handle;
	// podByUID is then a batch-local map filled by kwok_uid_lookup, and List pages go through
	// kwok_ingest_pods_framed_uid.  podUID / podRef (handle -> uid / name, for addressing patches) stay
	byUID       bool
	// refDir (KWOK_REF_DIR=1, with KWOK_UID_DIR=1 and KWOK_ECHO_LEDGER=1): the engine's reference directory
	// (kwok_watch.h, DESIGN.md §25) holds what a patch is addressed to; podUID, podRef and nodeName stay
	// empty: tickApply addresses every body with the reference the tick hands back, setupCNI asks
	// kwok_refs_lookup, the typed paths name their pods with kwok_refs_bind (bindBatch)
	refDir      bool
	batchRefs   map[types.UID]types.NamespacedName // refDir: the typed batch's names by uid (bindBatch)
	// nodeDir (KWOK_NODE_DIR=1, with the three switches above): the engine's node uid directory (kwok_watch.h,
	// DESIGN.md §26) holds a uid per node slot and resolves names to handles in batches (kwok_node_lookup);
	// nodeHandle stays empty too: typed pod events resolve spec.nodeName per run, typed node events bind
	// their uids with kwok_node_bind (this source has no relist sweep; controller.py's takes the swept
	// nodes' uids from kwok_refs_lookup)
	nodeDir     bool
	gpuCodec    bool // pod documents decoded on the GPU (kwok_ingest_pods_json); KWOK_GPU_CODEC=0: the host codec
	// nodeStatusGPU (KWOK_NODE_STATUS_GPU=1, with the GPU codec): the device canonicalises the status blobs of
	// the node documents it decodes (kwok_canon.h, DESIGN.md §28): a relist of nodes kwok has patched leaves
	// no document to the host codec
	nodeStatusGPU bool
	podDocsHost int  // pod documents the GPU codec left to the host codec (logged)
	nodeDocsHost int // node documents the GPU codec left to the host codec (logged)
}

func newGPUController(conf Config, interval time.Duration) (*GPUController, error) {
	st, err := time.Parse(time.RFC3339, startTime) // the StartTime() value (controller.go:33)
	if err != nil {
		return nil, err
	}
	eng, err := newGPUEngine(conf, st.Unix(), 0, 1, nil)
	if err != nil {
		return nil, err
	}
	codec, err := newGPUCodec(conf)
	if err != nil {
		eng.close()
		return nil, err
	}
	byUID := os.Getenv("KWOK_UID_DIR") == "1"
	if byUID {
		if err := eng.uidDirEnable(); err != nil {
			codec.close()
			eng.close()
			return nil, err
		}
	}
	var ledger *gpuEngine
	if os.Getenv("KWOK_ECHO_LEDGER") == "1" {
		if !byUID {
			codec.close()
			eng.close()
			return nil, fmt.Errorf("KWOK_ECHO_LEDGER=1 needs KWOK_UID_DIR=1")
		}
		if err := eng.echoEnable(); err != nil {
			codec.close()
			eng.close()
			return nil, err
		}
		ledger = eng
	}
	refDir := os.Getenv("KWOK_REF_DIR") == "1"
	if refDir {
		if !byUID || ledger == nil {
			codec.close()
			eng.close()
			return nil, fmt.Errorf("KWOK_REF_DIR=1 needs KWOK_UID_DIR=1 and KWOK_ECHO_LEDGER=1")
		}
		if err := eng.refsEnable(); err != nil {
			codec.close()
			eng.close()
			return nil, err
		}
	}
	nodeDir := os.Getenv("KWOK_NODE_DIR") == "1"
	if nodeDir {
		if !refDir {
			codec.close()
			eng.close()
			return nil, fmt.Errorf("KWOK_NODE_DIR=1 needs KWOK_UID_DIR=1, KWOK_ECHO_LEDGER=1 and KWOK_REF_DIR=1")
		}
		if err := eng.nodeDirEnable(); err != nil {
			codec.close()
			eng.close()
			return nil, err
		}
	}
	gpuCodecOn := os.Getenv("KWOK_GPU_CODEC") != "0"
	nodeStatusGPU := os.Getenv("KWOK_NODE_STATUS_GPU") == "1"
	if nodeStatusGPU {
		if !gpuCodecOn {
			codec.close()
			eng.close()
			return nil, fmt.Errorf("KWOK_NODE_STATUS_GPU=1 needs the GPU codec (KWOK_GPU_CODEC is 0)")
		}
		if err := eng.canonEnable(true); err != nil {
			codec.close()
			eng.close()
			return nil, err
		}
	}
	return &GPUController{
		byUID: byUID, refDir: refDir, nodeDir: nodeDir, batchRefs: map[types.UID]types.NamespacedName{},
		nodeStatusGPU: nodeStatusGPU,
		conf: conf, eng: eng, codec: codec, interval: interval, finalizer: finalizerPatch(),
		nodeName: map[int32]string{}, nodeHandle: map[string]int32{}, podByUID: map[types.UID]int32{},
		podUID: map[int32]types.UID{},
		podRef: map[int32]types.NamespacedName{},
		echo:     echoes{rv: map[types.UID][]string{}, ledger: ledger},
		queued:   map[types.UID]struct{}{},
		gpuCodec: gpuCodecOn,
	}, nil
}

// Start: the node and pod watches of NodeController.Start / PodController.Start
// (node_controller.go:119-143, pod_controller.go:130-153) feed the batches; the
// tick loop replaces KeepNodeHeartbeat, LockNodes, LockPods and DeletePods.
func (c *GPUController) Start(ctx context.Context) error {
	nodeOpt := metav1.ListOptions{LabelSelector: c.conf.ManageNodesWithLabelSelector}
	podOpt := metav1.ListOptions{FieldSelector: podFieldSelector}
	// KWOK_GPU_LIST=1: what exists is listed in pages first (ListNodes / ListPods at
	// Start, node_controller.go:282-296, pod_controller.go:357-368), each page framed
	// on the GPU and ingested in place; the watches then open from the lists'
	// resourceVersion.  Otherwise the watches open without one and the apiserver
	// replays every object as an Added event - unpaged, and not served for 10M pods.
	if os.Getenv("KWOK_GPU_LIST") == "1" {
		rv, err := c.listInto(ctx, true, nodeOpt)
		if err != nil {
			return fmt.Errorf("failed to list nodes: %w", err)
		}
		nodeOpt.ResourceVersion = rv
		if rv, err = c.listInto(ctx, false, podOpt); err != nil {
			return fmt.Errorf("failed to list pods: %w", err)
		}
		podOpt.ResourceVersion = rv
	}
	if err := c.watch(ctx, true, nodeOpt); err != nil {
		return fmt.Errorf("failed to watch nodes: %w", err)
	}
	if err := c.watch(ctx, false, podOpt); err != nil {
		return fmt.Errorf("failed to watch pods: %w", err)
	}
	go c.loop(ctx)
	return nil
}

// listPageSize: the pager's default (client-go tools/pager: 500)
const listPageSize = 500

// listInto pages through the kind's List with Limit and Continue, taking each
// page's raw body (DoRaw: no typed decode), frames it on the GPU
// (kwok_frame_list_gpu) and ingests its items from the resident body as upserts
// (kwok_ingest_nodes_framed / kwok_ingest_pods_framed).  It runs before the tick
// loop starts, so it owns the engine.  Returns the list's resourceVersion for
// the watch.  Objects absent from the list are not deleted.
func (c *GPUController) listInto(ctx context.Context, nodes bool, opt metav1.ListOptions) (string, error) {
	resource := "pods"
	if nodes {
		resource = "nodes"
	}
	opt.Limit = listPageSize
	text := func(body []byte, s C.kwok_str, escaped bool) (string, error) {
		raw := body[s.off : s.off+s.len]
		if !escaped {
			return string(raw), nil
		}
		var out string
		err := json.Unmarshal(append(append([]byte{'"'}, raw...), '"'), &out)
		return out, err
	}
	rv := ""
	for {
		body, err := c.conf.ClientSet.CoreV1().RESTClient().Get().Resource(resource).
			VersionedParams(&opt, scheme.ParameterCodec).DoRaw(ctx)
		if err != nil {
			return "", err
		}
		frames, info, staged, sid, err := c.eng.frameList(body)
		if err != nil {
			return "", err
		}
		idx, hs := make([]uint32, 0, len(frames)), make([]int32, 0, len(frames))
		for i := range frames {
			f := &frames[i]
			h := int32(-1)
			if !nodes && !c.byUID {
				uid, err := text(staged, f.uid, f.flags&C.KWOK_FRAME_ESC_UID != 0)
				if err != nil {
					return "", err
				}
				if known, ok := c.podByUID[types.UID(uid)]; ok {
					h = known
				}
			}
			idx, hs = append(idx, uint32(i)), append(hs, h)
		}
		var out, ss []int32
		if nodes {
			out, ss, err = c.eng.ingestNodesFramed(c.codec, sid, idx)
		} else if c.byUID { // uids resolved and creates bound on the device: no handle array, no map
			out, ss, _, err = c.eng.ingestPodsFramedUID(c.codec, sid, idx)
		} else {
			out, ss, err = c.eng.ingestPodsFramed(c.codec, sid, idx, hs)
		}
		if err != nil {
			return "", err
		}
		for k, i := range idx {
			if ss[k] != C.KWOK_OK {
				continue // outside the engine's domain (DESIGN.md §2)
			}
			if c.refDir && !nodes && frames[i].flags&(C.KWOK_FRAME_ESC_NAME|C.KWOK_FRAME_ESC_NS) == 0 {
				continue // (only an item whose name holds an escape is looked at: its decoded text is bound below)
			}
			f := &frames[i]
			name, err := text(staged, f.name, f.flags&C.KWOK_FRAME_ESC_NAME != 0)
			if err != nil {
				return "", err
			}
			if nodes {
				c.putNode(out[k], name)
				continue
			}
			if c.refDir { // an escaped name: the device stored none, the decoded text is bound
				ns, err := text(staged, f.namespace_, f.flags&C.KWOK_FRAME_ESC_NS != 0)
				if err != nil {
					return "", err
				}
				if _, err := c.eng.refsBind([]int32{out[k]}, []string{ns}, []string{name}); err != nil {
					return "", err
				}
				continue
			}
			ns, err := text(staged, f.namespace_, f.flags&C.KWOK_FRAME_ESC_NS != 0)
			if err != nil {
				return "", err
			}
			uid, _ := text(staged, f.uid, f.flags&C.KWOK_FRAME_ESC_UID != 0)
			if !c.byUID {
				c.podByUID[types.UID(uid)] = out[k]
			}
			c.podUID[out[k]] = types.UID(uid)
			c.podRef[out[k]] = types.NamespacedName{Namespace: ns, Name: name}
		}
		if rv, err = text(staged, info.resource_version, info.flags&C.KWOK_LIST_ESC_RV != 0); err != nil {
			return "", err
		}
		if opt.Continue, err = text(staged, info.continue_, info.flags&C.KWOK_LIST_ESC_CONTINUE != 0); err != nil {
			return "", err
		}
		if opt.Continue == "" {
			return rv, nil
		}
	}
}

// watch from the current state (a watch without resourceVersion first sends an
// Added event per existing object, as ListNodes / ListPods would), re-opened
// when the server closes it, like WatchNodes / WatchPods
func (c *GPUController) watch(ctx context.Context, nodes bool, opt metav1.ListOptions) error {
	open := func() (watch.Interface, error) {
		if nodes {
			return c.conf.ClientSet.CoreV1().Nodes().Watch(ctx, opt)
		}
		return c.conf.ClientSet.CoreV1().Pods(corev1.NamespaceAll).Watch(ctx, opt)
	}
	w, err := open()
	if err != nil {
		return err
	}
	logger := log.FromContext(ctx)
	go func() {
		rc := w.ResultChan()
		for {
			select {
			case <-ctx.Done():
				w.Stop()
				return
			case ev, ok := <-rc:
				if !ok {
					for {
						if w, err = open(); err == nil {
							rc = w.ResultChan()
							break
						}
						logger.Error("Failed to re-watch", err)
						select {
						case <-ctx.Done():
							return
						case <-time.After(time.Second * 5):
						}
					}
					continue
				}
				c.onEvent(ctx, nodes, ev)
			}
		}
	}()
	return nil
}

func (c *GPUController) onEvent(ctx context.Context, nodes bool, ev watch.Event) {
	if ev.Type != watch.Added && ev.Type != watch.Modified && ev.Type != watch.Deleted {
		return
	}
	var w watchObj
	switch obj := ev.Object.(type) {
	case *corev1.Node:
		if !nodes {
			return
		}
		w = watchObj{obj, obj.UID, obj.ResourceVersion, ev.Type == watch.Deleted}
	case *corev1.Pod:
		if nodes {
			return
		}
		w = watchObj{obj, obj.UID, obj.ResourceVersion, ev.Type == watch.Deleted}
	default:
		return
	}
	c.mu.Lock()
	defer c.mu.Unlock()
	// the echo of one of the engine's own patches (its apply already returned):
	// not queued, not encoded - unless another event of the object waits in this
	// tick's batch: that one is a change the engine has not seen, older than the
	// patch, and the echo is the object's newest state, carrying both
	_, waiting := c.queued[w.uid]
	if ev.Type == watch.Modified && c.echo.is(w.uid, w.rv) && !waiting {
		return
	}
	c.queued[w.uid] = struct{}{}
	if nodes {
		c.nodes = append(c.nodes, w)
	} else {
		c.pods = append(c.pods, w)
	}
}

func (c *GPUController) loop(ctx context.Context) {
	logger := log.FromContext(ctx)
	tasks := newParallelTasks(16) // the reference's heartbeat / lock / delete parallelism
	t := time.NewTimer(c.interval)
	defer func() {
		t.Stop()
		tasks.Wait()
		c.codec.close()
		c.eng.close()
	}()
	for {
		select {
		case <-ctx.Done():
			return
		case <-t.C:
			start := time.Now()
			n, err := c.step(ctx, tasks, start.Unix())
			tasks.Wait()
			if err != nil {
				logger.Error("Failed to tick", err)
			}
			logger.Info("Tick", "bodies", n, "elapsed", time.Since(start))
			t.Reset(c.interval)
		}
	}
}

// Has / Size: NodeController.Has / Size (node_controller.go:403-409) of the
// engine's managed-node set
func (c *GPUController) Has(nodeName string) bool { return c.eng.nodeHas(nodeName) }
func (c *GPUController) Size() int               { return c.eng.nodeSize() }

// step: ingest the batches (nodes first, so new pods find their node), give
// the tick's pending pods their CNI IPs (EnableCNI), run the tick, hand every
// body to the task pool; then the same interval again for the pods patched
// without a podIP (created with an empty status: pod.status.tpl renders no IPs
// then, `{{ with .status }}`).  In the reference that patch's own Modified event
// re-enters lockPodChan (pod_controller.go:279-319) and the pod gets hostIP /
// podIP at once; here the object the patch returned is ingested as that event
// (its watch echo is dropped like every echo) and the engine ticks again at the
// same clock, applying that tick's pod patches, node inits and deletes but not
// its heartbeats (the interval's heartbeats were sent).
func (c *GPUController) step(ctx context.Context, tasks *parallelTasks, now int64) (int, error) {
	c.mu.Lock()
	nw, pw := c.nodes, c.pods
	c.nodes, c.pods, c.queued = nil, nil, map[types.UID]struct{}{}
	c.mu.Unlock()
	// every apply of the previous tick has returned (loop waits for the task pool):
	// the echoes that overtook their patch's response are dropped here (ledger: the previous tick's
	// notes and forgets go to the device first)
	if err := c.echo.flush(); err != nil {
		return 0, err
	}
	nb, _, err := c.echo.encode(nw)
	if err != nil {
		return 0, err
	}
	pb, _, err := c.echo.encode(pw)
	if err != nil {
		return 0, err
	}
	if err := c.flushNodes(ctx, nb); err != nil {
		return 0, err
	}
	if err := c.flushPods(ctx, tasks, pb); err != nil {
		return 0, err
	}
	if c.conf.EnableCNI {
		if err := c.setupCNI(ctx, tasks); err != nil {
			return 0, err
		}
	}
	var re reentry
	n, err := c.tickApply(ctx, tasks, now, true, &re)
	for round := 0; round < 4 && err == nil; round++ { // (a re-entered pod's second patch carries its IPs)
		tasks.Wait()
		if len(re.objs) == 0 {
			break
		}
		var b objBatch
		for _, p := range re.objs {
			if err = b.add(watchObj{p, p.UID, p.ResourceVersion, false}); err != nil {
				return n, err
			}
		}
		re.objs = nil
		if err = c.flushPods(ctx, tasks, b); err != nil {
			return n, err
		}
		if c.conf.EnableCNI {
			if err = c.setupCNI(ctx, tasks); err != nil {
				return n, err
			}
		}
		var m int
		m, err = c.tickApply(ctx, tasks, now, false, &re)
		n += m
	}
	return n, err
}

// reentry: the objects returned by pod patches that carried no podIP
type reentry struct {
	mu   sync.Mutex
	objs []*corev1.Pod
}

var podIPKey = []byte(`"podIP"`)

// tickApply: one tick at now, every body handed to the task pool (heartbeats
// only when asked); pod patches without a podIP leave their returned object in re
func (c *GPUController) tickApply(ctx context.Context, tasks *parallelTasks, now int64, heartbeats bool,
	re *reentry) (int, error) {
	logger := log.FromContext(ctx)
	nodesAPI := c.conf.ClientSet.CoreV1().Nodes()
	var gone []int32
	n := 0
	err := c.eng.tick(now, func(kind int, h int32, body []byte, r *objRef) {
		if kind == kindHeartbeat && !heartbeats {
			return
		}
		if r != nil && r.status != C.KWOK_OK { // refDir: no name stored, the body cannot be addressed
			logger.Warn("No reference for an engine body", fmt.Errorf("kwok status %d", r.status))
			return
		}
		n++
		switch kind {
		case kindHeartbeat, kindNodeInit: // configureHeartbeatNode / configureNode bodies
			name := c.nodeName[h]
			if r != nil {
				name = r.name
			}
			tasks.Add(func() {
				n, err := nodesAPI.PatchStatus(ctx, name, body)
				if err != nil {
					logger.Error("Failed to patch node status", err, "node", name)
					return
				}
				c.echo.note(n.UID, n.ResourceVersion)
			})
		case kindPodPatch: // LockPod (pod_controller.go:205-231)
			ref := c.podRef[h]
			if r != nil {
				ref = types.NamespacedName{Namespace: r.namespace, Name: r.name}
			}
			tasks.Add(func() {
				p, err := c.conf.ClientSet.CoreV1().Pods(ref.Namespace).Patch(ctx, ref.Name,
					types.StrategicMergePatchType, body, metav1.PatchOptions{}, "status")
				if err != nil {
					if !apierrors.IsNotFound(err) {
						logger.Error("Failed to lock pod", err, "pod", ref.String())
					}
					return
				}
				c.echo.note(p.UID, p.ResourceVersion)
				if !bytes.Contains(body, podIPKey) { // an empty status: its echo re-enters
					re.mu.Lock()
					re.objs = append(re.objs, p)
					re.mu.Unlock()
				}
			})
		case kindDelete, kindDeleteFin: // DeletePod (pod_controller.go:155-183); the engine freed the handle
			ref, fin, uid := c.podRef[h], kind == kindDeleteFin, c.podUID[h]
			if r != nil {
				ref, uid = types.NamespacedName{Namespace: r.namespace, Name: r.name}, types.UID(r.uid)
			}
			gone = append(gone, h)
			// the pod's noted echoes go here, before the task: the echo its finalizer
			// patch notes (whenever the task runs) is then dropped, not re-ingested
			c.echo.forget(uid)
			tasks.Add(func() {
				pods := c.conf.ClientSet.CoreV1().Pods(ref.Namespace)
				if fin { // only pods with finalizers (len(pod.Finalizers) != 0, :161)
					p, err := pods.Patch(ctx, ref.Name, types.MergePatchType, c.finalizer, metav1.PatchOptions{})
					if err != nil {
						if !apierrors.IsNotFound(err) {
							logger.Error("Failed to patch pod finalizers", err, "pod", ref.String())
						}
						return
					}
					// its echo (deletionTimestamp, no finalizers) would re-enter DeletePod
					// for a pod the engine already deleted
					c.echo.note(p.UID, p.ResourceVersion)
				}
				if err := pods.Delete(ctx, ref.Name, deleteOpt); err != nil && !apierrors.IsNotFound(err) {
					logger.Error("Failed to delete pod", err, "pod", ref.String())
				}
			})
		}
	})
	for _, h := range gone { // the later Deleted watch event finds no handle (CNI: it still runs cni.Remove)
		delete(c.podByUID, c.podUID[h])
		delete(c.podUID, h)
		delete(c.podRef, h)
	}
	return n, err
}

// setupCNI: configurePod's cni.Setup for the pods the next tick evaluates that
// hold no podIP (pod_controller.go:383-389), 16 at a time; the engine patches
// them with the first returned IP.  A failed Setup leaves the pod unpatched
// this tick, as configurePod's error does.
func (c *GPUController) setupCNI(ctx context.Context, tasks *parallelTasks) error {
	hs, err := c.eng.cniPending()
	if err != nil || len(hs) == 0 {
		return err
	}
	logger := log.FromContext(ctx)
	ips := make([]uint32, len(hs))
	var named []objRef
	if c.refDir { // the pods that wait for an address, by the names the device holds
		if named, err = c.eng.refsLookup(C.KWOK_KIND_PODS, hs, 0); err != nil {
			return err
		}
	}
	for i, h := range hs {
		i, uid, ref := i, c.podUID[h], c.podRef[h]
		if c.refDir {
			if named[i].status != C.KWOK_OK {
				continue
			}
			uid, ref = types.UID(named[i].uid), types.NamespacedName{Namespace: named[i].namespace, Name: named[i].name}
		}
		tasks.Add(func() {
			got, err := cni.Setup(ctx, string(uid), ref.Name, ref.Namespace)
			if err != nil {
				logger.Error("cni setup", err, "pod", ref.String())
				return
			}
			if ip := net.ParseIP(got[0]).To4(); ip != nil {
				ips[i] = binary.BigEndian.Uint32(ip)
			}
		})
	}
	tasks.Wait()
	keep, kept := hs[:0], ips[:0]
	for i := range hs {
		if ips[i] != 0 {
			keep, kept = append(keep, hs[i]), append(kept, ips[i])
		}
	}
	return c.eng.cniAssign(keep, kept)
}

// flushNodes: the batch's node documents decoded on the GPU (kwok_ingest_nodes_json:
// a Deleted event's status is not read; a non-empty addresses / allocatable /
// capacity blob goes to the host codec inside the call) and routed by the GPU
// event switch; flushNodesHost decodes on the host (KWOK_GPU_CODEC=0).
// kwok_amd/controller.py _flush_nodes_gpu is this function in Python.
func (c *GPUController) flushNodes(ctx context.Context, b objBatch) error {
	if len(b.offs) == 0 {
		return nil
	}
	if !c.gpuCodec {
		return c.flushNodesHost(ctx, b)
	}
	logger := log.FromContext(ctx)
	ops := make([]uint8, len(b.offs))
	for i := range ops {
		ops[i] = C.KWOK_OP_UPSERT
		if b.del[i] {
			ops[i] = C.KWOK_OP_DELETE
		}
	}
	hs, ss, nHost, err := c.eng.ingestNodesJSON(c.codec, b.arena, b.offs, b.lens, ops)
	if err != nil {
		return err
	}
	c.nodeDocsHost += nHost
	bound := map[int32]string{} // nodeDir: handle -> the uid of its last upsert (a typed event carries none to the device)
	for i := range ops {
		if ss[i] != C.KWOK_OK {
			if ss[i] == C.KWOK_EDOMAIN || ss[i] == C.KWOK_EINVAL { // outside the engine's domain (DESIGN.md §2)
				logger.Warn("Node outside the supported domain", fmt.Errorf("kwok status %d", ss[i]))
			}
			continue
		}
		name := b.refs[i].Name
		if b.del[i] {
			delete(c.nodeName, hs[i])
			delete(c.nodeHandle, name)
			delete(bound, hs[i])
		} else {
			c.putNode(hs[i], name)
			bound[hs[i]] = string(b.uids[i])
		}
	}
	if c.nodeDir {
		bh, bu := make([]int32, 0, len(bound)), make([]string, 0, len(bound))
		for h, u := range bound {
			if len(u) > 0 && len(u) <= C.KWOK_UID_MAX {
				bh, bu = append(bh, h), append(bu, u)
			}
		}
		if _, err := c.eng.nodeBind(bh, bu); err != nil {
			return err
		}
	}
	return nil
}

// putNode: a node the engine created or updated - its handle by name and, without the reference directory,
// its name by handle
func (c *GPUController) putNode(h int32, name string) {
	if c.nodeDir { // (the device holds the name, the handle and the uid)
		return
	}
	if !c.refDir {
		c.nodeName[h] = name
	}
	c.nodeHandle[name] = h
}

// putPod: a pod the engine created or updated - its uid and name by handle (refDir: the device holds them;
// the typed batch's names are kept by uid for bindBatch)
func (c *GPUController) putPod(h int32, uid types.UID, ref types.NamespacedName) {
	if c.refDir {
		c.batchRefs[uid] = ref
		return
	}
	c.podUID[h] = uid
	c.podRef[h] = ref
}

// flushNodesHost: flushNodes with the host codec (kwok_decode_nodes)
func (c *GPUController) flushNodesHost(ctx context.Context, b objBatch) error {
	logger := log.FromContext(ctx)
	ev, st := c.codec.decodeNodes(b.arena, b.offs, b.lens, runtime.NumCPU())
	keep := make([]C.kwok_node_event, 0, len(ev))
	names := make([]string, 0, len(ev))
	for i := range ev {
		if st[i] != C.KWOK_OK { // outside the engine's domain: not simulated (DESIGN.md §2)
			logger.Warn("Node outside the supported domain", fmt.Errorf("kwok status %d", st[i]))
			continue
		}
		ev[i].op = C.KWOK_OP_UPSERT
		if b.del[i] {
			ev[i].op = C.KWOK_OP_DELETE
		}
		keep = append(keep, ev[i])
		names = append(names, str(b.arena, ev[i].name))
	}
	hs, ss, err := c.eng.ingestNodes(keep, b.arena)
	if err != nil {
		return err
	}
	for i := range keep {
		if ss[i] != C.KWOK_OK {
			continue
		}
		if keep[i].op == C.KWOK_OP_DELETE {
			delete(c.nodeName, hs[i])
			delete(c.nodeHandle, names[i])
		} else {
			c.putNode(hs[i], names[i])
		}
	}
	return nil
}

// flushPods ingests the batch in event order.  A pod's first event in the
// batch may create it (handle -1); its later events need that handle, so the
// batch is cut into runs in which no new pod appears twice: run k+1 is
// ingested after run k, once run k's handles are known.  (Added then Modified,
// or Added then Deleted, within one interval: one slot, then its update or its
// Deleted event with the pod's podIP release, pod_controller.go:329-336.)
// flushPods: the batch's pod documents decoded on the GPU (kwok_ingest_pods_json)
// in runs in which no new pod appears twice - a pod's first event may create it
// and its later events need that handle (Added + Modified, Added + Deleted in one
// interval) - the same runs as flushPodsHost, which decodes on the host
// (kwok_decode_pods) and is kept for engines built without the device codec
// (kwok_amd/controller.py ingest_doc_runs is this function in Python)
func (c *GPUController) flushPods(ctx context.Context, tasks *parallelTasks, b objBatch) error {
	if len(b.offs) == 0 {
		return nil
	}
	if !c.gpuCodec {
		if c.byUID { // (the same bracket as below around the host-codec runs)
			if err := c.lookupBatch(b.uids); err != nil {
				return err
			}
			defer func() { c.podByUID = map[types.UID]int32{} }()
			if err := c.flushPodsHost(ctx, tasks, b); err != nil {
				return err
			}
			return c.bindBatch()
		}
		return c.flushPodsHost(ctx, tasks, b)
	}
	logger := log.FromContext(ctx)
	if c.byUID {
		// the batch's uids resolved by the device: podByUID holds this batch's known pods only, the runs
		// below update it, and the pods it ends with are bound (typed events and raw bytes of one pod mix)
		if err := c.lookupBatch(b.uids); err != nil {
			return err
		}
		defer func() { c.podByUID = map[types.UID]int32{} }()
	}
	var run []int
	created := map[types.UID]bool{} // new pods of the current run
	flush := func() error {
		offs, lens := make([]uint64, 0, len(run)), make([]uint32, 0, len(run))
		ops, hs := make([]uint8, 0, len(run)), make([]int32, 0, len(run))
		keep := run[:0]
		for _, i := range run {
			h, known := c.podByUID[b.uids[i]]
			if b.del[i] {
				// EnableCNI: cni.Remove for a pod on a managed node (pod_controller.go:337-342),
				// also when the engine deleted it already (its handle is gone)
				if c.conf.EnableCNI && c.eng.nodeHas(b.nodes[i]) {
					uid, ref := b.uids[i], b.refs[i]
					tasks.Add(func() {
						if err := cni.Remove(context.Background(), string(uid), ref.Name, ref.Namespace); err != nil {
							logger.Error("cni remove", err)
						}
					})
				}
				if !known { // never ingested, or already deleted by the engine
					continue
				}
				ops = append(ops, C.KWOK_OP_DELETE) // releases status.podIP (pod_controller.go:329-336)
				hs = append(hs, h)
			} else {
				ops = append(ops, C.KWOK_OP_UPSERT)
				if !known {
					h = -1
				}
				hs = append(hs, h)
			}
			offs, lens = append(offs, b.offs[i]), append(lens, b.lens[i])
			keep = append(keep, i)
		}
		run = run[:0]
		for k := range created {
			delete(created, k)
		}
		out, ss, nHost, err := c.eng.ingestPodsJSON(c.codec, b.arena, offs, lens, ops, hs)
		if err != nil {
			return err
		}
		c.podDocsHost += nHost
		for k, i := range keep {
			if ss[k] != C.KWOK_OK {
				logger.Warn("Pod outside the supported domain", fmt.Errorf("kwok status %d", ss[k]))
				continue
			}
			uid := b.uids[i]
			if ops[k] == C.KWOK_OP_DELETE {
				delete(c.podByUID, uid)
				delete(c.podUID, out[k])
				delete(c.podRef, out[k])
			} else {
				c.podByUID[uid] = out[k]
				c.putPod(out[k], uid, b.refs[i])
			}
		}
		return nil
	}
	for i := range b.offs {
		uid := b.uids[i]
		if created[uid] { // its handle comes from the run before
			if err := flush(); err != nil {
				return err
			}
		}
		if _, known := c.podByUID[uid]; !known && !b.del[i] {
			created[uid] = true
		}
		run = append(run, i)
	}
	if err := flush(); err != nil {
		return err
	}
	if c.byUID {
		return c.bindBatch()
	}
	return nil
}

// lookupBatch (byUID): podByUID = the batch's uids the directory holds (kwok_uid_lookup)
func (c *GPUController) lookupBatch(uids []types.UID) error {
	seen := map[types.UID]struct{}{}
	us := make([]types.UID, 0, len(uids))
	for _, u := range uids {
		if _, ok := seen[u]; !ok {
			seen[u] = struct{}{}
			us = append(us, u)
		}
	}
	hs, err := c.eng.uidLookup(us)
	if err != nil {
		return err
	}
	c.podByUID = map[types.UID]int32{}
	for i, u := range us {
		if hs[i] >= 0 {
			c.podByUID[u] = hs[i]
		}
	}
	return nil
}

// bindBatch (byUID): the pods the batch-local map ends with are bound on the device (kwok_uid_bind); a uid
// the directory cannot key (empty, longer than KWOK_UID_MAX) is left out and stays unknown to it
func (c *GPUController) bindBatch() error {
	hs, us := make([]int32, 0, len(c.podByUID)), make([]types.UID, 0, len(c.podByUID))
	for u, h := range c.podByUID {
		if len(u) > 0 && len(u) <= C.KWOK_UID_MAX {
			hs, us = append(hs, h), append(us, u)
		}
	}
	if _, err := c.eng.uidBind(hs, us); err != nil || !c.refDir {
		return err
	}
	// refDir: ... and named (a typed event carries neither its uid nor its name to the device)
	hs = hs[:0]
	nss, names := make([]string, 0, len(c.batchRefs)), make([]string, 0, len(c.batchRefs))
	for u, ref := range c.batchRefs {
		if h, ok := c.podByUID[u]; ok && len(ref.Name) > 0 && len(ref.Name) <= C.KWOK_REF_NAME_MAX && len(ref.Namespace) <= C.KWOK_REF_NS_MAX {
			hs, nss, names = append(hs, h), append(nss, ref.Namespace), append(names, ref.Name)
		}
	}
	c.batchRefs = map[types.UID]types.NamespacedName{}
	_, err := c.eng.refsBind(hs, nss, names)
	return err
}

// flushPodsHost: flushPods with the host codec (kwok_decode_pods) and the packed
// wire forms (ingestPods)
func (c *GPUController) flushPodsHost(ctx context.Context, tasks *parallelTasks, b objBatch) error {
	logger := log.FromContext(ctx)
	docs, st := c.codec.decodePods(b.arena, b.offs, b.lens, runtime.NumCPU())
	type rec struct {
		i   int // index in the batch
		ref types.NamespacedName
	}
	var run []rec
	created := map[types.UID]bool{} // new pods of the current run
	flush := func() error {
		evs := make([]C.kwok_pod_event, 0, len(run))
		keep := run[:0]
		on := c.nodeHandle // name -> handle of the nodes the engine holds
		if c.nodeDir {     // ... resolved for the run's names by one kwok_node_lookup
			on = map[string]int32{}
			var names []string
			for _, r := range run {
				if nm := str(b.arena, docs[r.i].ev.node_name); !b.del[r.i] {
					if _, seen := on[nm]; !seen {
						on[nm] = -1
						names = append(names, nm)
					}
				}
			}
			nhs, err := c.eng.nodeLookup(names)
			if err != nil {
				return err
			}
			for k, nm := range names {
				if nhs[k] >= 0 {
					on[nm] = nhs[k]
				} else {
					delete(on, nm)
				}
			}
		}
		for _, r := range run {
			d := &docs[r.i]
			h, known := c.podByUID[b.uids[r.i]]
			if b.del[r.i] {
				// EnableCNI: cni.Remove for a pod on a managed node (pod_controller.go:337-342),
				// also when the engine deleted it already (its handle is gone)
				if c.conf.EnableCNI && c.eng.nodeHas(str(b.arena, d.ev.node_name)) {
					uid, ref := b.uids[r.i], r.ref
					tasks.Add(func() {
						if err := cni.Remove(context.Background(), string(uid), ref.Name, ref.Namespace); err != nil {
							logger.Error("cni remove", err)
						}
					})
				}
				if !known { // never ingested, or already deleted by the engine
					continue
				}
				d.ev.op = C.KWOK_OP_DELETE // releases status.podIP (pod_controller.go:329-336)
				d.ev.handle = C.int32_t(h)
			} else {
				id, err := c.eng.registerPodSpec(d, b.arena)
				if err != nil {
					logger.Warn("Pod spec outside the supported domain", err)
					continue
				}
				d.ev.op = C.KWOK_OP_UPSERT
				d.ev.handle = -1
				if known {
					d.ev.handle = C.int32_t(h)
				}
				d.ev.spec_id = C.int32_t(id)
				// the node by handle when the engine holds it (no name lookup on the host);
				// otherwise by spec.nodeName (a deleted node pods still reference, or none yet)
				d.ev.node_handle = -1
				if nh, ok := on[str(b.arena, d.ev.node_name)]; ok {
					d.ev.node_handle = C.int32_t(nh)
				}
			}
			evs = append(evs, d.ev)
			keep = append(keep, r)
		}
		run = run[:0]
		for k := range created {
			delete(created, k)
		}
		hs, ss, _, err := c.eng.ingestPods(evs, b.arena)
		if err != nil {
			return err
		}
		for k, r := range keep {
			if ss[k] != C.KWOK_OK {
				continue
			}
			uid := b.uids[r.i]
			if evs[k].op == C.KWOK_OP_DELETE {
				delete(c.podByUID, uid)
				delete(c.podUID, hs[k])
				delete(c.podRef, hs[k])
			} else {
				c.podByUID[uid] = hs[k]
				c.putPod(hs[k], uid, r.ref)
			}
		}
		return nil
	}
	for i := range docs {
		if st[i] != C.KWOK_OK {
			logger.Warn("Pod outside the supported domain", fmt.Errorf("kwok status %d", st[i]))
			continue
		}
		uid := b.uids[i]
		if created[uid] { // its handle comes from the run before
			if err := flush(); err != nil {
				return err
			}
		}
		if _, known := c.podByUID[uid]; !known && !b.del[i] {
			created[uid] = true
		}
		d := &docs[i]
		run = append(run, rec{i, types.NamespacedName{Namespace: str(b.arena, d.namespace_), Name: str(b.arena, d.name)}})
	}
	return flush()
}
