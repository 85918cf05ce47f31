/*
 * oracle/rt_oracle_mesh.inc -- TEST INFRASTRUCTURE, included by rt_oracle.c.
 * Restatement of the reference's triangle-mesh path: OBJ loader
 * (/root/reference/kernel.cu:575-747), flat BVH build (:752-937, getMinMaxP
 * :971-995), Moller-Trumbore test (:1024-1059). SURVEY.md 8(f) row 4.
 */
typedef struct {
    o_cube box;      /* Bvhbox::bvhbox = new cube(c1, c2), kernel.cu:515-520 */
    int *indexes;
    int length;
} bvhbox_t;

struct o_mesh {
    o_triangle *tris;
    int poly_count;
    bvhbox_t *boxes;
    int bvhbox_count;
    int has_normals;
};

typedef struct { void *p; int n, cap; size_t esz; } vecbuf;
static void vb_init(vecbuf *v, size_t esz) { v->p = NULL; v->n = v->cap = 0; v->esz = esz; }
static void *vb_push(vecbuf *v)
{
    if (v->n == v->cap) {
        v->cap = v->cap ? v->cap * 2 : 64;
        v->p = realloc(v->p, (size_t)v->cap * v->esz);
    }
    return (char *)v->p + (size_t)(v->n++) * v->esz;
}

/* SlashCount, kernel.cu:1063-1070 */
static int SlashCount(const char *s)
{
    int c = 0;
    for (; *s; ++s) if (*s == '/') c++;
    return c;
}

/* splitString + operator>>: the '/'-separated integers of one face token
 * ("7/3/5" -> 7 3 5, "7//5" -> 7 5), kernel.cu:1072-1108 */
static int split_ints(const char *tok, int *out, int max)
{
    int n = 0;
    const char *p = tok;
    while (*p && n < max) {
        while (*p == '/' || *p == ' ') p++;
        if (!*p) break;
        char *end;
        long v = strtol(p, &end, 10);
        if (end == p) break;
        out[n++] = (int)v;
        p = end;
    }
    return n;
}

static o_triangle make_tri(vec3d p0, vec3d p1, vec3d p2, vec3d n0, vec3d n1, vec3d n2,
                           float u0, float v0, float u1, float v1, float u2, float v2)
{
    o_triangle t;
    vec3d e1 = sub(&p1, &p0), e2 = sub(&p2, &p0);
    vec3d nrm = cross(&e1, &e2);      /* cross(sub(p[f1],p[f0]), sub(p[f2],p[f0])) */
    nrm = normalise(&nrm);
    t.points[0] = p0; t.points[1] = p1; t.points[2] = p2;
    t.normal = nrm;
    t.vecNormal[0] = n0; t.vecNormal[1] = n1; t.vecNormal[2] = n2;
    t.vt[0][0] = u0; t.vt[0][1] = v0; t.vt[1][0] = u1; t.vt[1][1] = v1; t.vt[2][0] = u2; t.vt[2][1] = v2;
    return t;
}

/* getMinMaxP, kernel.cu:971-995 */
static void getMinMaxP(const o_triangle *tri, vec3d *min, vec3d *max)
{
    for (int j = 0; j < 3; j++) {
        if (tri->points[j].x > max->x) max->x = tri->points[j].x;
        if (tri->points[j].y > max->y) max->y = tri->points[j].y;
        if (tri->points[j].z > max->z) max->z = tri->points[j].z;
        if (tri->points[j].x < min->x) min->x = tri->points[j].x;
        if (tri->points[j].y < min->y) min->y = tri->points[j].y;
        if (tri->points[j].z < min->z) min->z = tri->points[j].z;
    }
}

static bvhbox_t make_box(vec3d c1, vec3d c2, int *idx, int len)
{
    bvhbox_t b;
    oracle_make_cube(&b.box, c1.x, c1.y, c1.z, c2.x, c2.y, c2.z);
    b.indexes = idx;
    b.length = len;
    return b;
}

/* createBvhMesh, kernel.cu:752-937: ten passes; every box with more than 5
 * triangles is split at the midpoint of its bounds along an axis that advances
 * (y, x, z, y, ...) after EVERY split, by the triangle's first vertex. */
static void createBvhMesh(o_mesh *m)
{
    const o_triangle *T = m->tris;
    int n = m->poly_count;
    vecbuf prev, temp;
    vb_init(&prev, sizeof(bvhbox_t));
    vb_init(&temp, sizeof(bvhbox_t));
    int splitDir = 0;

    vec3d lowestP = T[0].points[0];
    vec3d highestP = T[n - 1].points[0];
    for (int i = 0; i < n; i++) getMinMaxP(&T[i], &lowestP, &highestP);
    int *all = (int *)malloc(sizeof(int) * (size_t)n);
    for (int i = 0; i < n; i++) all[i] = i;
    *(bvhbox_t *)vb_push(&prev) = make_box(lowestP, highestP, all, n);

    for (int layer = 0; layer < 10; layer++) {        /* bvhLayer_count = 10, kernel.cu:570 */
        for (int j = 0; j < prev.n; j++) {
            bvhbox_t pb = ((bvhbox_t *)prev.p)[j];
            if (pb.length > 5) {
                int *i1 = (int *)malloc(sizeof(int) * (size_t)pb.length), n1 = 0;
                int *i2 = (int *)malloc(sizeof(int) * (size_t)pb.length), n2 = 0;
                float splitP;
                if (splitDir == 0) splitP = (pb.box.bounds[1].y + pb.box.bounds[0].y) / 2;
                else if (splitDir == 1) splitP = (pb.box.bounds[1].x + pb.box.bounds[0].x) / 2;
                else splitP = (pb.box.bounds[1].z + pb.box.bounds[0].z) / 2;
                for (int z = 0; z < pb.length; z++) {
                    const vec3d *p0 = &T[pb.indexes[z]].points[0];
                    float key = splitDir == 0 ? p0->y : splitDir == 1 ? p0->x : p0->z;
                    if (key <= splitP) i1[n1++] = pb.indexes[z];
                    else i2[n2++] = pb.indexes[z];
                }
                if (n1 != 0) {
                    vec3d low = T[i1[0]].points[0], high = T[i1[n1 - 1]].points[0];
                    for (int z = 0; z < n1; z++) getMinMaxP(&T[i1[z]], &low, &high);
                    *(bvhbox_t *)vb_push(&temp) = make_box(low, high, i1, n1);
                } else free(i1);
                if (n2 != 0) {
                    vec3d low = T[i2[0]].points[0], high = T[i2[n2 - 1]].points[0];
                    for (int z = 0; z < n2; z++) getMinMaxP(&T[i2[z]], &low, &high);
                    *(bvhbox_t *)vb_push(&temp) = make_box(low, high, i2, n2);
                } else free(i2);
                splitDir = (splitDir == 0 ? 1 : splitDir == 1 ? 2 : 0);
            } else {
                *(bvhbox_t *)vb_push(&temp) = pb;
            }
        }
        free(prev.p);
        prev = temp;
        vb_init(&temp, sizeof(bvhbox_t));
    }
    m->boxes = (bvhbox_t *)prev.p;
    m->bvhbox_count = prev.n;
}

/* mesh(string filename), kernel.cu:575-747, on the text of the file */
o_mesh *oracle_mesh_from_obj(const char *text)
{
    vecbuf P, VN, VT, TR;
    vb_init(&P, sizeof(vec3d)); vb_init(&VN, sizeof(vec3d)); vb_init(&VT, 2 * sizeof(float));
    vb_init(&TR, sizeof(o_triangle));
    int has_normals = 0;
    const char *cur = text;
    while (*cur) {
        const char *eol = strchr(cur, '\n');
        size_t len = eol ? (size_t)(eol - cur) : strlen(cur);
        char line[512];
        if (len >= sizeof line) len = sizeof line - 1;
        memcpy(line, cur, len);
        line[len] = 0;
        if (len && line[len - 1] == '\r') line[--len] = 0;
        cur = eol ? eol + 1 : cur + len;
        const char *s = line;
        while (*s == ' ' || *s == '\t') s++;
        if (!*s) continue;                       /* blank line: skipped (deviation, see header) */
        char c = *s;                             /* ss >> c */
        char type = len > 1 ? line[1] : 0;       /* char type = line[1] */
        if (c == 'v' || c == 'V') {
            if (type == 'n' || type == 'N') {    /* ss >> junk >> n.x >> n.y >> n.z */
                vec3d n = { 0, 0, 0 };
                sscanf(s + 2, "%f %f %f", &n.x, &n.y, &n.z);
                *(vec3d *)vb_push(&VN) = n;
            } else if (type == 't' || type == 'T') {
                float uv[2] = { 0, 0 };
                sscanf(s + 2, "%f %f", &uv[0], &uv[1]);
                memcpy(vb_push(&VT), uv, sizeof uv);
            } else {
                vec3d v = { 0, 0, 0 };
                sscanf(s + 1, "%f %f %f", &v.x, &v.y, &v.z);
                *(vec3d *)vb_push(&P) = v;
            }
        }
        if (c == 'f' || c == 'F') {
            char in[4][64] = { "", "", "", "" };
            int ntok = sscanf(s + 1, "%63s %63s %63s %63s", in[0], in[1], in[2], in[3]);
            if (ntok < 3) continue;
            const vec3d *p = (const vec3d *)P.p, *vn = (const vec3d *)VN.p;
            const float(*vt)[2] = (const float(*)[2])VT.p;
            int slashes = SlashCount(line);
            int f[4] = { 0 }, a[4] = { 0 }, b[4] = { 0 }, tmp[3];
            vec3d zero = { 0, 0, 0 };
#define PIDX(k) p[f[k] - 1]
            if (VN.n != 0 && VT.n != 0) {
                for (int k = 0; k < 4 && k < ntok; k++) {
                    tmp[0] = tmp[1] = tmp[2] = 0;
                    split_ints(in[k], tmp, 3);
                    f[k] = tmp[0]; a[k] = tmp[1]; b[k] = tmp[2];   /* >> f >> pvt >> pvn */
                }
                if (slashes <= 6)
                    *(o_triangle *)vb_push(&TR) = make_tri(PIDX(0), PIDX(1), PIDX(2), vn[b[0] - 1], vn[b[1] - 1], vn[b[2] - 1],
                        vt[a[0] - 1][0], vt[a[0] - 1][1], vt[a[1] - 1][0], vt[a[1] - 1][1], vt[a[2] - 1][0], vt[a[2] - 1][1]);
                if (slashes >= 8) {
                    o_triangle t1 = make_tri(PIDX(0), PIDX(1), PIDX(2), vn[b[0] - 1], vn[b[1] - 1], vn[b[2] - 1],
                        vt[a[0] - 1][0], vt[a[0] - 1][1], vt[a[1] - 1][0], vt[a[1] - 1][1], vt[a[2] - 1][0], vt[a[2] - 1][1]);
                    /* second half: points 0,2,3 but the FIRST triangle's face normal, and
                     * vt[pvt[2]] twice (kernel.cu:672) */
                    o_triangle t2 = make_tri(PIDX(0), PIDX(2), PIDX(3), vn[b[0] - 1], vn[b[2] - 1], vn[b[3] - 1],
                        vt[a[0] - 1][0], vt[a[0] - 1][1], vt[a[2] - 1][0], vt[a[2] - 1][1], vt[a[2] - 1][0], vt[a[2] - 1][1]);
                    t2.normal = t1.normal;
                    *(o_triangle *)vb_push(&TR) = t1;
                    *(o_triangle *)vb_push(&TR) = t2;
                }
                has_normals = 1;
            } else if (VN.n != 0) {
                for (int k = 0; k < 4 && k < ntok; k++) {
                    tmp[0] = tmp[1] = 0;
                    split_ints(in[k], tmp, 2);
                    f[k] = tmp[0]; b[k] = tmp[1];                  /* >> f >> pvn */
                }
                if (slashes <= 6)
                    *(o_triangle *)vb_push(&TR) = make_tri(PIDX(0), PIDX(1), PIDX(2), vn[b[0] - 1], vn[b[1] - 1], vn[b[2] - 1],
                                                           0, 0, 0, 1, 1, 0);
                if (slashes >= 8) {
                    o_triangle t1 = make_tri(PIDX(0), PIDX(1), PIDX(2), vn[b[0] - 1], vn[b[1] - 1], vn[b[2] - 1], 0, 0, 0, 1, 1, 0);
                    /* kernel.cu:710: the second half reuses vn[pvn[0..2]] */
                    o_triangle t2 = make_tri(PIDX(0), PIDX(2), PIDX(3), vn[b[0] - 1], vn[b[1] - 1], vn[b[2] - 1], 0, 0, 0, 1, 1, 0);
                    t2.normal = t1.normal;
                    *(o_triangle *)vb_push(&TR) = t1;
                    *(o_triangle *)vb_push(&TR) = t2;
                }
                has_normals = 1;
            } else {
                for (int k = 0; k < 4 && k < ntok; k++) f[k] = atoi(in[k]);   /* stoi(in[k]) */
                if (slashes <= 6)
                    *(o_triangle *)vb_push(&TR) = make_tri(PIDX(0), PIDX(1), PIDX(2), zero, zero, zero,
                        (float)0.666413, (float)0.250594, (float)0.333587, (float)0.250594, (float)0.333587, (float)0.000975);
                if (slashes == 8) {
                    o_triangle t1 = make_tri(PIDX(0), PIDX(1), PIDX(2), zero, zero, zero, 0, 0, 0, 1, 1, 0);
                    o_triangle t2 = make_tri(PIDX(0), PIDX(2), PIDX(3), zero, zero, zero, 0, 0, 0, 1, 1, 0);
                    t2.normal = t1.normal;
                    *(o_triangle *)vb_push(&TR) = t1;
                    *(o_triangle *)vb_push(&TR) = t2;
                }
                has_normals = 0;
            }
#undef PIDX
        }
    }
    free(P.p); free(VN.p); free(VT.p);
    if (TR.n == 0) { free(TR.p); return NULL; }
    o_mesh *m = (o_mesh *)calloc(1, sizeof *m);
    m->tris = (o_triangle *)TR.p;
    m->poly_count = TR.n;
    m->has_normals = has_normals;
    createBvhMesh(m);
    return m;
}

void oracle_mesh_free(o_mesh *m)
{
    if (!m) return;
    free(m->tris);
    free(m->boxes);   /* index arrays are shared between layers; leaked on purpose (test tool) */
    free(m);
}

int oracle_mesh_counts(const o_mesh *m, int *poly_count, int *bvhbox_count, int *has_normals)
{
    if (!m) return 1;
    if (poly_count) *poly_count = m->poly_count;
    if (bvhbox_count) *bvhbox_count = m->bvhbox_count;
    if (has_normals) *has_normals = m->has_normals;
    return 0;
}
const o_triangle *oracle_mesh_triangles(const o_mesh *m) { return m ? m->tris : NULL; }
int oracle_mesh_box(const o_mesh *m, int j, float bounds[6], float orgin[3], const int **indexes, int *length)
{
    if (!m || j < 0 || j >= m->bvhbox_count) return 1;
    const bvhbox_t *b = &m->boxes[j];
    bounds[0] = b->box.bounds[0].x; bounds[1] = b->box.bounds[0].y; bounds[2] = b->box.bounds[0].z;
    bounds[3] = b->box.bounds[1].x; bounds[4] = b->box.bounds[1].y; bounds[5] = b->box.bounds[1].z;
    orgin[0] = b->box.orgin.x; orgin[1] = b->box.orgin.y; orgin[2] = b->box.orgin.z;
    *indexes = b->indexes;
    *length = b->length;
    return 0;
}

/* Test aid, not a restatement: every leaf becomes consecutive leaves of at most max_len triangles, in the same
 * order, each with the bounds createBvhMesh gives a leaf of those triangles (first vertex of its first and last
 * triangle, grown by getMinMaxP). A mesh of more leaves than the ten passes can make (2^10), which a caller may
 * still hand to the product. The new leaves point into the old index arrays. */
int oracle_mesh_split_leaves(o_mesh *m, int max_len)
{
    if (!m || max_len < 1) return 1;
    const o_triangle *T = m->tris;
    vecbuf out;
    vb_init(&out, sizeof(bvhbox_t));
    for (int j = 0; j < m->bvhbox_count; j++) {
        const bvhbox_t *b = &m->boxes[j];
        for (int c0 = 0; c0 < b->length; c0 += max_len) {
            int *idx = b->indexes + c0;
            int len = b->length - c0 < max_len ? b->length - c0 : max_len;
            vec3d low = T[idx[0]].points[0], high = T[idx[len - 1]].points[0];
            for (int z = 0; z < len; z++) getMinMaxP(&T[idx[z]], &low, &high);
            *(bvhbox_t *)vb_push(&out) = make_box(low, high, idx, len);
        }
    }
    free(m->boxes);
    m->boxes = (bvhbox_t *)out.p;
    m->bvhbox_count = out.n;
    return 0;
}

/* mesh::rayIntersect (Moller-Trumbore), kernel.cu:1024-1059 */
static int rayIntersect(const ray *r, const o_triangle *tri, float *t, float *u, float *v)
{
    vec3d edge1 = sub(&tri->points[1], &tri->points[0]);
    vec3d edge2 = sub(&tri->points[2], &tri->points[0]);
    vec3d h, s, q;
    float a, f;

    h = cross(&r->Dir, &edge2);
    a = dotproduct(&edge1, &h);

    if (a > -0.0000001f && (double)a < 0.0000001)   /* float literal, then double literal */
        return 0;

    f = 1.f / a;

    s = sub(&r->Org, &tri->points[0]);
    *u = f * dotproduct(&s, &h);

    if (*u < 0.f || *u > 1.f)
        return 0;

    q = cross(&s, &edge1);
    *v = f * dotproduct(&r->Dir, &q);
    if (*v < 0.f || *u + *v > 1.f)
        return 0;

    *t = f * dotproduct(&edge2, &q);
    if ((double)*t > 0.0000001)
        return 1;
    return 0;
}

int oracle_triangle_intersect(const o_triangle *tri, const o_ray *r, float *t, float *u, float *v)
{
    return rayIntersect(r, tri, t, u, v);
}
